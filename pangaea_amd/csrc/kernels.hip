// kernels.hip -- gfx950 kernels of the barcode k-mer feature path + their C-ABI launchers.
//
// Replaces (reference file:line, /root/reference/src):
//   K2  pg_kmer_count*            jellyfish count -C (feature.py:94) + dump reload (cpptools/count_kmer.cpp:139-170)
//   K1  pg_features / tnf         cpptools/count_tnf.cpp:78-113  (per-run canonical k_tnf-mer counts)
//   K3  pg_features / abd         cpptools/count_kmer.cpp:55-108 (per-run histogram of global multiplicities), by table lookups
//       pg_abundance_from_records the same rows without random HBM reads, from the partitioned occurrence records
//
// Work decomposition (wave64):
//   * the read stream is 2-bit codes + 1-bit validity, 32 characters per word (include/pangaea_feat.h);
//     one lane owns one word per step, so a wave reads 512 B of codes + 256 B of validity, coalesced;
//   * a lane rolls the forward and reverse-complement codes over its 32 characters after pre-rolling
//     the k-1 characters before its word (taken from the previous word), so no cross-lane traffic;
//   * which positions end a valid k-mer comes from one bit-parallel pass over the 64-bit validity
//     window (runs of >= k ones), not from a per-character run counter;
//   * integer counting only: LDS histograms / LDS hash tables, global atomics only where unavoidable.
//     No MFMA -- there is no contraction on this path.
//
// Hash table building, two ways:
//   direct    (kmer_count_kernel)      one random 64-B line + one memory-side atomic per k-mer occurrence;
//   bucketed  (pg_kmer_count_bucketed) occurrences are hash-partitioned by two streaming scatter passes (LDS-staged so
//             HBM sees whole runs), every bucket is then counted inside LDS by one workgroup and its LDS image is
//             written back as that bucket's slice of the table.  HBM only sees streams; counting atomics are LDS atomics.
// Abundance rows, two ways:
//   lookups   (features_kernel)        one random 64-B line per k-mer occurrence;
//   shuffle   (pg_abundance_from_records) the partition records carry their row id; every bucket's slice is loaded into
//             LDS, each record's count becomes a (row, bin) word, the words are scattered back by row group (two passes)
//             and histogrammed in LDS.  Again only streams.
#include "pg_device.hpp"

namespace {
enum { TK_NONE = 0, TK_DENSE = 1, TK_HASH = 2, TK_WIDE = 3, TK_MINI = 4, TK_MINIW = 5 };

// (key42, the slot key of the packed hash tables, and its inverse: pg_device.hpp)

// hash table as the kernels see it: 2^log2_slots slots in buckets of 2^log2_bucket slots; a key's home slot is its top
// log2_slots bits (packed form) / the top bits of mix64(code) (wide form), probing is linear and wraps inside the
// bucket.  Slots are never freed, so a lookup may stop at the first empty slot.
struct HashView {
    uint64_t *slots;
    int log2_slots;
    int log2_bucket;
    __device__ __forceinline__ uint64_t home_wide(uint64_t code) const { return mix64(code) >> (64 - log2_slots); }
    __device__ __forceinline__ uint64_t home_key(uint64_t key) const { return key >> (KEY_BITS - log2_slots); }
    // PG_TABLE_MINI: bucket from the k-mer's minimizer, slot inside the bucket from a hash of the code (the slots hold codes)
    __device__ __forceinline__ uint64_t home_mini(uint64_t code, int k) const
    {
        const uint32_t b = mini_bucket(mini_minimizer_of(code, k), log2_slots - log2_bucket);
        return ((uint64_t)b << log2_bucket) | (mini_slot_hash<true>(code) & ((1u << log2_bucket) - 1u));
    }
    __device__ __forceinline__ uint64_t next(uint64_t s) const
    {
        const uint64_t bm = (1ull << log2_bucket) - 1;
        return (s & ~bm) | ((s + 1) & bm);
    }
    __device__ __forceinline__ uint32_t limit() const { return log2_bucket < 14 ? (1u << log2_bucket) : MAX_PROBE; }
};

template <typename KT> __device__ __forceinline__ KT low_mask(int k)
{
    return (2 * k >= (int)(8 * sizeof(KT))) ? (KT)~(KT)0 : (KT)(((KT)1 << (2 * k)) - 1);
}

// rolling state of one lane: forward / reverse-complement code of the last k characters
template <typename KT> struct Roller {
    KT fw, rc, kmask;
    int rc_shift;
    __device__ __forceinline__ void init(int k)
    {
        fw = rc = 0;
        kmask = low_mask<KT>(k);
        rc_shift = 2 * (k - 1);
    }
    __device__ __forceinline__ void push(uint32_t c)
    {
        fw = (KT)(fw << 2) | (KT)c;
        rc = (KT)(rc >> 2) | (KT)((KT)(c ^ 2u) << rc_shift);
    }
    __device__ __forceinline__ KT canon() const
    {
        const KT f = fw & kmask;
        return f < rc ? f : rc;
    }
};

// -------------------------------------------------------------------------------- table access

__device__ __forceinline__ void dense_add(uint32_t *table, uint32_t code) { atomicAdd(&table[code], 1u); }

// slot = (key << 22) | count, key = key42(code) ; 0 = empty.  Keys never change once written, so a stale (cached)
// read can only show "empty", and the compare-and-swap then returns the real occupant.
__device__ __forceinline__ void hash_add_from(const HashView &t, uint64_t s, uint64_t cur, uint64_t code, uint32_t *status)
{
    const uint32_t limit = t.limit();
    for (uint32_t i = 0; i < limit; ++i) {
        if (cur == 0) {
            cur = atomicCAS((unsigned long long *)&t.slots[s], 0ull, (unsigned long long)((code << HASH_CBITS) | 1ull));
            if (cur == 0) return;
        }
        if ((cur >> HASH_CBITS) == code) {
            // stop growing at SAT; overshoot is bounded by the threads in flight (< 2^20 < 2^22 - SAT)
            if ((uint32_t)(cur & HASH_CMASK) < HASH_SAT) atomicAdd((unsigned long long *)&t.slots[s], 1ull);
            return;
        }
        s = t.next(s);
        cur = t.slots[s];
    }
    atomicOr(status, 1u);
}

__device__ __forceinline__ uint32_t hash_probe(const HashView &t, uint64_t s, uint64_t cur, uint64_t code, bool *found)
{
    const uint32_t limit = t.limit();
    for (uint32_t i = 0; i < limit; ++i) {
        if (cur == 0) break;
        if ((cur >> HASH_CBITS) == code) { *found = true; return (uint32_t)(cur & HASH_CMASK); }
        s = t.next(s);
        cur = t.slots[s];
    }
    *found = false;
    return 0;
}

// Wide form (k <= 31): keys[2^s] hold code + 1 (0 = empty), counts[2^s] (uint32) follow the key array.  Same placement
// and probing as the packed form; counts wrap modulo 2^32 like any uint32 counter.
__device__ __forceinline__ uint32_t *wide_counts(const HashView &t) { return reinterpret_cast<uint32_t *>(t.slots + (1ull << t.log2_slots)); }

// (mini_k != 0: a PG_TABLE_MINI_WIDE table -- home slot from the minimizer bucket, same keys/counts planes)
__device__ __forceinline__ void wide_add(const HashView &t, uint64_t code, uint32_t add, uint32_t *status, int mini_k = 0)
{
    const uint32_t limit = t.limit();
    const uint64_t key1 = code + 1;
    uint64_t s = mini_k ? t.home_mini(code, mini_k) : t.home_wide(code);
    for (uint32_t i = 0; i < limit; ++i) {
        uint64_t cur = t.slots[s];
        if (cur == 0) {
            cur = atomicCAS((unsigned long long *)&t.slots[s], 0ull, (unsigned long long)key1);
            if (cur == 0) cur = key1;
        }
        if (cur == key1) { atomicAdd(&wide_counts(t)[s], add); return; }
        s = t.next(s);
    }
    atomicOr(status, 1u);
}

__device__ __forceinline__ uint32_t wide_probe(const HashView &t, uint64_t s, uint64_t cur, uint64_t code, bool *found)
{
    const uint32_t limit = t.limit();
    const uint64_t key1 = code + 1;
    for (uint32_t i = 0; i < limit; ++i) {
        if (cur == 0) break;
        if (cur == key1) { *found = true; return wide_counts(t)[s]; }
        s = t.next(s);
        cur = t.slots[s];
    }
    *found = false;
    return 0;
}

__global__ __launch_bounds__(BLOCK) void wide_merge_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ counts, int64_t n,
                                                           HashView t, uint32_t *status, int mini_k)
{
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK)
        if (counts[i]) wide_add(t, codes[i], counts[i], status, mini_k);
}

// -------------------------------------------------------------------------------- K2 direct: global counts

template <typename KT, int TK>
__global__ __launch_bounds__(BLOCK) void kmer_count_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                           int64_t word_begin, int64_t word_end, int k, uint32_t *dense,
                                                           HashView t, uint32_t *status)
{
    for (int64_t w = word_begin + (int64_t)blockIdx.x * BLOCK + threadIdx.x; w < word_end; w += (int64_t)gridDim.x * BLOCK) {
        const Word x = load_word(codes, valid, w, k);
        if (x.ok == 0) continue;
        Roller<KT> r;
        r.init(k);
        for (int i = 33 - k; i < 32; ++i) r.push((uint32_t)(x.pw >> (2 * i)) & 3u);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            KT canon[8];
            uint64_t cur[8];
            uint64_t hh[8];
            uint64_t kk[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = b * 8 + u;
                r.push((uint32_t)(x.cw >> (2 * j)) & 3u);
                canon[u] = r.canon();
                if ((x.ok >> j) & 1) {
                    if (TK == TK_DENSE) {
                        dense_add(dense, (uint32_t)canon[u]);
                    } else if (TK == TK_WIDE) {
                        wide_add(t, (uint64_t)canon[u], 1u, status);
                    } else {                       // issue the first probe of the whole batch before resolving any
                        kk[u] = key42((uint64_t)canon[u]);
                        hh[u] = t.home_key(kk[u]);
                        cur[u] = t.slots[hh[u]];
                    }
                }
            }
            if (TK == TK_HASH) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if ((x.ok >> (b * 8 + u)) & 1) hash_add_from(t, hh[u], cur[u], kk[u], status);
            }
        }
    }
}

// merge (key,count) pairs of another table (slot format); counts saturate at SAT exactly (CAS loop; not a hot path)
__global__ __launch_bounds__(BLOCK) void kmer_merge_kernel(const uint64_t *__restrict__ pairs, int64_t n, HashView t, uint32_t *status, int mini_k)
{
    const uint32_t limit = t.limit();
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
        const uint64_t p = pairs[i];
        if (p == 0) continue;
        const uint64_t code = p >> HASH_CBITS;
        uint32_t add = (uint32_t)(p & HASH_CMASK);
        if (add > HASH_SAT) add = HASH_SAT;
        uint64_t s = mini_k ? t.home_mini(code, mini_k) : t.home_key(code);
        bool done = false;
        for (uint32_t tries = 0; tries < limit && !done; ++tries) {
            uint64_t cur = __hip_atomic_load(&t.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                if (cur != 0 && (cur >> HASH_CBITS) != code) break;          // occupied by another key
                uint32_t have = (uint32_t)(cur & HASH_CMASK);
                uint32_t sum = have + add > HASH_SAT ? HASH_SAT : have + add;
                uint64_t want = (code << HASH_CBITS) | sum;
                uint64_t old = atomicCAS((unsigned long long *)&t.slots[s], (unsigned long long)cur, (unsigned long long)want);
                if (old == cur) { done = true; break; }
                cur = old;
            }
            s = t.next(s);
        }
        if (!done) atomicOr(status, 1u);
    }
}

// -------------------------------------------------------------------------------- reading a finished table
//
// What `jellyfish query` and `jellyfish histo` answer from the dump that the reference keeps (feature.py:87,103).  Both kernels
// only read the table: plain loads, no atomics on it.

// out[i] = multiplicity of the k-mer codes[i] (either strand; the stream's encoding, newest character in the low bits), 0 when
// the table does not hold it, PG_QUERY_INVALID when the code has a bit at or above 2k -- such a code reads no table memory.
// One query per lane and turn, QRY_BATCH turns at a time: the first probes of the batch are issued before any is resolved
// (every probe is a random 8-byte read, i.e. one 64-byte line, as the lookups of features_kernel).
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
// One streaming pass, 16 bytes per lane and load (SPEC_FORM: four dense counters, two packed slots, or four keys of the key
// plane with their four counts), SPEC_UNROLL loads in flight per lane.  Bins are 32-bit LDS counters (dynamic LDS, high + 2 of
// them: at most 64 KiB); a workgroup sees fewer than 2^32 slots (the launcher's grid), so none overflows.  Real spectra are
// mostly c == 1 (sequencing errors): all 64 lanes would add to one LDS counter, so those lanes are counted with a ballot and
// kept in a register of the wavefront until the end (BALLOT >= 1; BALLOT == 2: c == 2 as well); every other count is an LDS add
// whose result nobody reads.  Non-zero bins leave with one 64-bit global add each: integer sums, the same whatever the order.
enum { SPEC_DENSE = 0, SPEC_PACKED = 1, SPEC_PLANES = 2 };
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
                if (FORM == SPEC_PLANES) { v[q] = slots[2 * i]; w[q] = slots[2 * i + 1]; c[q] = counts[i]; }
                else v[q] = slots[i];
            }
        }
#pragma unroll
        for (int q = 0; q < SPEC_UNROLL; ++q) {
            if (FORM == SPEC_DENSE) {
                spectrum_bin<BALLOT>(bins, v[q].x, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, v[q].y, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, v[q].z, cap, ones, twos);
                spectrum_bin<BALLOT>(bins, v[q].w, cap, ones, twos);
            } else if (FORM == SPEC_PACKED) {
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
enum { DUMP_DENSE = 0, DUMP_HASH = 1, DUMP_MINI = 2, DUMP_PLANES = 3 };
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

// HyperLogLog sketch of the canonical k-mers of a word range: registers[j] = max over k-mers with hash prefix j of
// (1 + leading zeros of the remaining hash bits).  4096 registers: ~1.6 % standard error -- enough to size a table.
constexpr int HLL_BITS = 12;
__global__ __launch_bounds__(BIG_BLOCK) void distinct_sketch_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                                    int64_t word_begin, int64_t word_end, int k, uint32_t *__restrict__ registers)
{
    __shared__ uint32_t reg[1 << HLL_BITS];
    for (int i = threadIdx.x; i < (1 << HLL_BITS); i += BIG_BLOCK) reg[i] = 0;
    __syncthreads();
    for (int64_t w = word_begin + (int64_t)blockIdx.x * BIG_BLOCK + threadIdx.x; w < word_end; w += (int64_t)gridDim.x * BIG_BLOCK) {
        const Word x = load_word(codes, valid, w, k);
        if (x.ok == 0) continue;
        Roller<uint64_t> r;
        r.init(k);
        for (int i = 33 - k; i < 32; ++i) r.push((uint32_t)(x.pw >> (2 * i)) & 3u);
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            r.push((uint32_t)(x.cw >> (2 * j)) & 3u);
            if ((x.ok >> j) & 1) {
                // an independent hash (the table's own hash decides bucket membership; reusing it would not bias the
                // sketch, but keeping them apart costs nothing)
                const uint64_t h = mix64(r.canon() ^ 0x9E3779B97F4A7C15ull);
                const uint32_t idx = (uint32_t)(h >> (64 - HLL_BITS));
                const uint64_t rest = (h << HLL_BITS) | (1ull << (HLL_BITS - 1));      // sentinel bit bounds the rank
                atomicMax(&reg[idx], (uint32_t)__clzll((long long)rest) + 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (1 << HLL_BITS); i += BIG_BLOCK)
        if (reg[i]) atomicMax(&registers[i], reg[i]);
}

// -------------------------------------------------------------------------------- partition machinery
//
// occurrence record = canonical code (low 42 bits) | row id << 42 (22 bits, ROW_NONE = not inside any row)

constexpr int RPL64 = 32, RPL32 = 32; // record scatter passes: 8-byte / 4-byte records a lane keeps in registers
constexpr int MAX_FAN_BITS = 9;       // <= 512-way scatter per pass
constexpr int WIDE_FAN_BITS = 10;     // the one-pass row shuffle: 1024 row groups (65536 rows), 64 words per lane
constexpr int RPL32_WIDE = 64;
constexpr int REC_KEY_BITS = 42;
constexpr uint64_t REC_KEY_MASK = (1ull << REC_KEY_BITS) - 1;
constexpr uint32_t ROW_NONE = (1u << (64 - REC_KEY_BITS)) - 1;
constexpr int GROUP_ROWS_LOG2 = 6;    // rows per LDS row-histogram group (64 x 512 bins x 4 B = 128 KiB at most)

constexpr int TILE_WORDS = 256;       // words per stream tile of the first scatter pass (= A1_TILE_WORDS)
// first row whose end lies beyond the first character of each stream tile (rows sorted, disjoint)
__global__ __launch_bounds__(BLOCK) void tile_rows_kernel(const int64_t *__restrict__ row_end, int64_t n_rows, int64_t word_begin,
                                                          int64_t n_tiles, int32_t *__restrict__ tile_row)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_tiles) return;
    const int64_t c0 = (word_begin + t * TILE_WORDS) * 32;
    int64_t lo = 0, hi = n_rows;                                    // first r with row_end[r] > c0
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_end[mid] > c0) hi = mid; else lo = mid + 1;
    }
    tile_row[t] = (int32_t)lo;
}

// A0: histogram of final bucket ids (top `bits` bits of the hash) over every valid k-mer of the word range; one launch
// covers the bins [bin_base, bin_base + n_bins) (n_bins <= 2^15: 128 KiB of LDS counters).  With chunk_hist given it
// also records, for every CHUNK_WORDS-word chunk of the range, how many k-mers fall into each first-pass digit
// (top bits1 bits): chunk_hist[d * n_chunks + chunk].  A per-digit scan of that table gives every chunk its exact write
// offsets, so the first scatter pass needs no global cursor atomics.
constexpr int CHUNK_WORDS = 4096;     // = 32 stream tiles of the first scatter pass
__global__ __launch_bounds__(BIG_BLOCK) void bucket_hist_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                                int64_t word_begin, int64_t word_end, int k, int bits,
                                                                uint32_t bin_base, int n_bins, unsigned long long *__restrict__ hist,
                                                                int bits1, unsigned long long *__restrict__ chunk_hist, int64_t n_chunks,
                                                                int64_t chunk_stride)
{
    // chunks are placed in the order slot = chunk * chunk_stride mod n_chunks (stride coprime to n_chunks): regions then
    // hold the stream in scrambled chunk order, so later passes do not see row-sorted input
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *coarse = lds + n_bins;                                // [256]
    for (int i = threadIdx.x; i < n_bins; i += BIG_BLOCK) lds[i] = 0;
    const int sh = KEY_BITS - bits, sh1 = KEY_BITS - bits1;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        if (threadIdx.x < 256) coarse[threadIdx.x] = 0;
        __syncthreads();
        const int64_t w0 = word_begin + chunk * CHUNK_WORDS;
        const int64_t w1 = w0 + CHUNK_WORDS < word_end ? w0 + CHUNK_WORDS : word_end;
        for (int64_t w = w0 + threadIdx.x; w < w1; w += BIG_BLOCK) {
            const Word x = load_word(codes, valid, w, k);
            if (x.ok == 0) continue;
            Roller<uint64_t> r;
            r.init(k);
            for (int i = 33 - k; i < 32; ++i) r.push((uint32_t)(x.pw >> (2 * i)) & 3u);
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                r.push((uint32_t)(x.cw >> (2 * j)) & 3u);
                if ((x.ok >> j) & 1) {
                    const uint64_t h = key42(r.canon());
                    const uint32_t bin = (uint32_t)(h >> sh) - bin_base;
                    if (bin < (uint32_t)n_bins) atomicAdd(&lds[bin], 1u);
                    if (chunk_hist) atomicAdd(&coarse[h >> sh1], 1u);
                }
            }
        }
        __syncthreads();
        if (chunk_hist && threadIdx.x < (1u << bits1))
            chunk_hist[(int64_t)threadIdx.x * n_chunks + (int64_t)(((__int128)chunk * chunk_stride) % n_chunks)] = coarse[threadIdx.x];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_bins; i += BIG_BLOCK)
        if (lds[i]) atomicAdd(&hist[bin_base + i], (unsigned long long)lds[i]);
}

// LDS bookkeeping shared by the scatter passes (<= 2^FAN_BITS digits)
template <int FAN_BITS> struct ScatterLds {
    uint32_t start[(1 << FAN_BITS) + 1];
    unsigned long long gbase[1 << FAN_BITS];                        // its first half doubles as the digit counters until the scan
    uint32_t wave_tot[WAVES];
    __device__ __forceinline__ uint32_t *cnt() { return reinterpret_cast<uint32_t *>(gbase); }
};

// exclusive scan of L.cnt[0..n_dig) into L.start[0..n_dig] (PER = 2^FAN_BITS / BLOCK consecutive entries per lane); all lanes call
template <int FAN_BITS> __device__ __forceinline__ void scatter_scan(ScatterLds<FAN_BITS> &L, int n_dig)
{
    constexpr int PER = (1 << FAN_BITS) / BLOCK > 0 ? (1 << FAN_BITS) / BLOCK : 1;
    uint32_t e[PER];
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = PER * (int)threadIdx.x + j;
        e[j] = i < n_dig ? L.cnt()[i] : 0;
        v += e[j];
    }
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if ((int)(threadIdx.x & 63) >= d) incl += o;
    }
    if ((threadIdx.x & 63) == 63) L.wave_tot[threadIdx.x >> 6] = incl;
    lds_sync();
    uint32_t before = 0;
    for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) before += L.wave_tot[wv];
    uint32_t run = before + incl - v;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int i = PER * (int)threadIdx.x + j;
        if (i < n_dig) L.start[i] = run;
        run += e[j];
    }
    if (threadIdx.x == BLOCK - 1) L.start[n_dig] = before + incl;
    lds_sync();
}

// A1: stream -> 2^bits1 regions (bits1 <= 8).  A lane owns HALF a word (16 characters) and keeps its <= 16 records in
// registers; one returning LDS atomic per record yields its rank inside its digit, the tile (128 words, <= 4096
// records) is then laid out digit-sorted in LDS and every digit's run is appended to its region with one global cursor
// add, so HBM receives contiguous runs.  36 KiB of LDS per workgroup: four workgroups (16 waves) per CU.
// With rows given, every record also carries the index of the row its k-mer ends in (ROW_NONE outside all rows).
constexpr int A1_CHARS = 32;            // characters per lane: 16 (two lanes share a word) or 32
constexpr int A1_LANES_PER_WORD = 32 / A1_CHARS;
constexpr int A1_TILE_WORDS = BLOCK * A1_CHARS / 32;
static_assert(A1_TILE_WORDS == TILE_WORDS, "tile_rows_kernel and scatter_stream_kernel must agree on the tile size");
constexpr int A1_TILE = BLOCK * A1_CHARS;
struct StreamLds {
    uint32_t cnt[256];
    uint32_t start[257];
    unsigned long long gbase[256];
    unsigned long long cur[256];                                    // running write offsets of this chunk, per digit
    uint32_t wave_tot[WAVES];
};
static_assert(CHUNK_WORDS % A1_TILE_WORDS == 0, "a chunk is a whole number of stream tiles");
__global__ __launch_bounds__(BLOCK) void scatter_stream_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                               int64_t word_begin, int64_t word_end, int k, int bits1,
                                                               const int64_t *__restrict__ row_start, const int64_t *__restrict__ row_end,
                                                               int64_t n_rows, const uint32_t *__restrict__ strict,
                                                               const int32_t *__restrict__ tile_row,
                                                               uint64_t *__restrict__ rec_out,
                                                               const unsigned long long *__restrict__ chunk_off, int64_t n_chunks,
                                                               int64_t chunk_stride)
{
    // one workgroup per chunk: chunk_off[d * n_chunks + chunk] is where this chunk's records of digit d start
    __shared__ uint64_t buf[A1_TILE];
    __shared__ StreamLds L;
    const int n_dig = 1 << bits1;
    const int dsh = KEY_BITS - bits1;
    const int64_t n_tiles = (word_end - word_begin + A1_TILE_WORDS - 1) / A1_TILE_WORDS;
    const int half = threadIdx.x % A1_LANES_PER_WORD;               // which A1_CHARS characters of the word
    const int64_t chunk = blockIdx.x;
    constexpr int TILES_PER_CHUNK = CHUNK_WORDS / A1_TILE_WORDS;
    const int64_t slot = (int64_t)(((__int128)chunk * chunk_stride) % n_chunks);
    if ((int)threadIdx.x < n_dig) L.cur[threadIdx.x] = chunk_off[(int64_t)threadIdx.x * n_chunks + slot];
    for (int64_t tile = chunk * TILES_PER_CHUNK; tile < (chunk + 1) * TILES_PER_CHUNK && tile < n_tiles; ++tile) {
        L.cnt[threadIdx.x] = 0;
        lds_sync();
        uint64_t rec[A1_CHARS];
        uint32_t dr[A1_CHARS];                                      // digit << 16 | rank inside the digit
        uint32_t ok = 0;
        const int64_t w = word_begin + tile * A1_TILE_WORDS + (threadIdx.x / A1_LANES_PER_WORD);
        if (w < word_end) {
            const Word x = load_word(codes, valid, w, k);
            ok = (uint32_t)(((uint64_t)x.ok >> (A1_CHARS * half)) & ((1ull << A1_CHARS) - 1ull));
            // `valid` may count lower-case bases as bases (jellyfish's rule for the table); the rows follow the reference's own
            // counters, which do not: with a second, strict validity plane a k-mer that is only valid under the lenient rule is
            // counted but belongs to no row
            uint32_t ok_row = ok;
            if (strict && ok) {
                const uint32_t sv = strict[w], sp = w > 0 ? strict[w - 1] : 0u;
                ok_row &= (uint32_t)(((runs_of(((uint64_t)sv << 32) | sp, k) >> 32) >> (A1_CHARS * half)) & ((1ull << A1_CHARS) - 1ull));
            }
            if (ok) {
                // row bookkeeping: r = first row that can still contain a position >= the current one
                int64_t r = n_rows, rs = INT64_MAX, re = INT64_MAX;
                const int64_t pos0 = (w << 5) + A1_CHARS * half;
                if (row_start) {
                    r = tile_row[tile];
                    while (r < n_rows && row_end[r] <= pos0) ++r;
                    if (r < n_rows) { rs = row_start[r]; re = row_end[r]; }
                }
                Roller<uint64_t> rl;
                rl.init(k);
                // pre-roll the k-1 characters before the lane's first one: word positions c in [first-(k-1), first)
                for (int c = A1_CHARS * half - (k - 1); c < A1_CHARS * half; ++c)
                    rl.push((uint32_t)((c < 0 ? x.pw >> (2 * (c + 32)) : x.cw >> (2 * c)) & 3u));
                const uint64_t mine = x.cw >> (2 * A1_CHARS * half);
#pragma unroll
                for (int j = 0; j < A1_CHARS; ++j) {
                    rl.push((uint32_t)(mine >> (2 * j)) & 3u);
                    if ((ok >> j) & 1) {
                        const int64_t pos = pos0 + j;
                        while (pos >= re) {                         // rows are at least one character long: terminates
                            ++r;
                            rs = r < n_rows ? row_start[r] : INT64_MAX;
                            re = r < n_rows ? row_end[r] : INT64_MAX;
                        }
                        const uint64_t row = (pos >= rs && ((ok_row >> j) & 1)) ? (uint64_t)r : (uint64_t)ROW_NONE;
                        const uint64_t key = key42(rl.canon());
                        const uint32_t d = (uint32_t)(key >> dsh);
                        rec[j] = key | (row << REC_KEY_BITS);
                        dr[j] = (d << 16) | atomicAdd(&L.cnt[d], 1u);
                    }
                }
            }
        }
        lds_sync();
        {   // exclusive scan of cnt[256] -> start[257]: one entry per lane
            const uint32_t v = L.cnt[threadIdx.x];
            uint32_t incl = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)(threadIdx.x & 63) >= d) incl += o;
            }
            if ((threadIdx.x & 63) == 63) L.wave_tot[threadIdx.x >> 6] = incl;
            lds_sync();
            uint32_t before = 0;
            for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) before += L.wave_tot[wv];
            L.start[threadIdx.x] = before + incl - v;
            if (threadIdx.x == BLOCK - 1) L.start[BLOCK] = before + incl;
            // gbase[d] = (where the digit's run goes) - (where it starts in the tile): the copy-out adds the tile position
            if ((int)threadIdx.x < n_dig) { L.gbase[threadIdx.x] = L.cur[threadIdx.x] - (before + incl - v); L.cur[threadIdx.x] += v; }
            lds_sync();
        }
#pragma unroll
        for (int j = 0; j < A1_CHARS; ++j)
            if ((ok >> j) & 1) buf[L.start[dr[j] >> 16] + (dr[j] & 0xffffu)] = rec[j];
        lds_sync();
        // copy out: LDS position i holds a record of digit d at rank i - start[d]; the digit is recomputed from the record
        // (pure ALU), so the loop is a flat, pipelinable sweep and consecutive lanes write consecutive addresses per run
        const uint32_t total = L.start[BLOCK];
        for (uint32_t i = threadIdx.x; i < total; i += BLOCK) {
            const uint64_t r = buf[i];
            const uint32_t d = (uint32_t)((r & REC_KEY_MASK) >> dsh);
            rec_out[L.gbase[d] + i] = r;
        }
        lds_sync();
    }
}

// Generic record scatter pass (A2, S2a, S2b).  Region = blockIdx.x / tiles_x; its input records are
//   [in_begin[region << in_shift], in_cnt ? begin + in_cnt[region] : in_end[region << in_shift]).
// Digit: DIG_HASH -> (key >> dshift) & mask of a (key, row) record;  DIG_ROW -> (word >> dshift) & mask of a 32-bit (row, bin) word.
// Destination of digit d: out[obase[(base + d) << oshift] + cursor[base + d] ...], base = flat ? 0 : region << dbits.
enum { DIG_HASH = 0, DIG_ROW = 1 };
template <typename REC, int DIG, int REC_PER_LANE, int FAN_BITS>
__global__ __launch_bounds__(BLOCK) void scatter_records_kernel(const REC *__restrict__ rec_in,
                                                                const unsigned long long *__restrict__ in_begin,
                                                                const unsigned long long *__restrict__ in_end, int in_shift,
                                                                const unsigned long long *__restrict__ in_cnt, int tiles_x,
                                                                REC *__restrict__ rec_out, const unsigned long long *__restrict__ obase,
                                                                unsigned long long *__restrict__ cursor, int oshift, int flat,
                                                                int dbits, int dshift)
{
    constexpr int TILE1 = BLOCK * REC_PER_LANE;
    __shared__ REC buf[TILE1];
    __shared__ ScatterLds<FAN_BITS> L;
    const int n_dig = 1 << dbits;
    const uint32_t dmask = (uint32_t)n_dig - 1u;
    // (all workgroups of a region on ONE of the eight XCDs, which take workgroups round-robin by index: the runs its tiles append
    // to a destination are completed in that XCD's L2 -- see mini_scatter2_kernel.  Flat destinations are shared by all regions.)
    const unsigned n_regions = gridDim.x / (unsigned)tiles_x;
    const bool by_xcd = !flat && n_regions % 8u == 0u;
    const int64_t region = by_xcd ? (int64_t)(blockIdx.x % 8u) + 8 * (int64_t)((blockIdx.x / 8u) / (unsigned)tiles_x) : (int64_t)(blockIdx.x / tiles_x);
    const int64_t base_index = flat ? 0 : (region << dbits);
    const int64_t r0 = (int64_t)in_begin[region << in_shift];
    const int64_t r1 = in_cnt ? r0 + (int64_t)in_cnt[region] : (int64_t)in_end[region << in_shift];
    const int64_t n_tiles = (r1 - r0 + TILE1 - 1) / TILE1;
    auto digit_of = [&](REC r) -> uint32_t {
        if (DIG == DIG_HASH) return (uint32_t)(((uint64_t)r & REC_KEY_MASK) >> dshift) & dmask;
        return ((uint32_t)r >> dshift) & dmask;
    };
    for (int64_t tile = by_xcd ? (blockIdx.x / 8u) % (unsigned)tiles_x : blockIdx.x % tiles_x; tile < n_tiles; tile += tiles_x) {
        for (int i = threadIdx.x; i < n_dig; i += BLOCK) L.cnt()[i] = 0;
        lds_sync();
        const int64_t t0 = r0 + tile * TILE1;
        REC rec[REC_PER_LANE];
        uint32_t dr[REC_PER_LANE];
#pragma unroll
        for (int j = 0; j < REC_PER_LANE; ++j) {                    // all loads of the lane in flight together
            const int64_t i = t0 + j * BLOCK + threadIdx.x;
            rec[j] = i < r1 ? rec_in[i] : (REC)0;
        }
#pragma unroll
        for (int j = 0; j < REC_PER_LANE; ++j) {
            const int64_t i = t0 + j * BLOCK + threadIdx.x;
            // (an all-ones word is a hole: a lookup pass that keeps its words in place marks dropped ones that way)
            if (i < r1 && !(DIG == DIG_ROW && (uint32_t)rec[j] == 0xffffffffu)) {
                const uint32_t d = digit_of(rec[j]);
                dr[j] = (d << 16) | atomicAdd(&L.cnt()[d], 1u);
            }
        }
        lds_sync();
        scatter_scan(L, n_dig);
        // the returning cursor adds (one per digit and tile) are issued first and consumed after the placement: their round
        // trip to L2 overlaps the LDS stores instead of standing in front of them
        constexpr int DPL = ((1 << FAN_BITS) + BLOCK - 1) / BLOCK;  // digits per lane
        unsigned long long gpos[DPL];
#pragma unroll
        for (int q = 0; q < DPL; ++q) {                             // cnt[] is gone (it shared gbase's storage): start[] has it
            const int d = (int)threadIdx.x + q * BLOCK;
            gpos[q] = 0;
            if (d < n_dig) {
                const uint32_t c = L.start[d + 1] - L.start[d];
                if (c) gpos[q] = obase[(base_index + d) << oshift] + atomicAdd(&cursor[base_index + d], (unsigned long long)c) - L.start[d];
            }
        }
#pragma unroll
        for (int j = 0; j < REC_PER_LANE; ++j) {
            const int64_t i = t0 + j * BLOCK + threadIdx.x;
            if (i < r1 && !(DIG == DIG_ROW && (uint32_t)rec[j] == 0xffffffffu)) buf[L.start[dr[j] >> 16] + (dr[j] & 0xffffu)] = rec[j];
        }
#pragma unroll
        for (int q = 0; q < DPL; ++q) {
            const int d = (int)threadIdx.x + q * BLOCK;
            if (d < n_dig) L.gbase[d] = gpos[q];
        }
        lds_sync();
        const uint32_t total = L.start[n_dig];
        for (uint32_t i = threadIdx.x; i < total; i += BLOCK) {    // flat sweep: digit recomputed from the record
            const REC r = buf[i];
            const uint32_t d = digit_of(r);
            rec_out[L.gbase[d] + i] = r;                            // gbase[d] = destination of the run - its start in the tile
        }
        lds_sync();
    }
}

// insert one record into the LDS table, starting from an already fetched first slot; false = table full
__device__ __forceinline__ bool lds_insert(unsigned long long *tab, uint32_t smask, uint32_t limit,
                                           uint64_t code, bool live, uint32_t s, unsigned long long cur)
{
    if (!live) return true;                                         // padding lane of the last batch
    for (uint32_t i = 0; i < limit; ++i) {
        if (cur == 0) {
            cur = atomicCAS(&tab[s], 0ull, (unsigned long long)((code << HASH_CBITS) | 1ull));
            if (cur == 0) return true;
        }
        if ((cur >> HASH_CBITS) == code) {
            if ((uint32_t)(cur & HASH_CMASK) < HASH_SAT) atomicAdd(&tab[s], 1ull);
            return true;
        }
        s = (s + 1) & smask;
        cur = tab[s];
    }
    return false;
}

// B: one workgroup per final bucket.  The bucket's slice of the table (2^log2_bucket slots) lives in LDS while the
// bucket's records stream through (8 loads per lane in flight, first LDS probes of a batch issued back to back);
// the LDS image is then written back as the slice.
constexpr int CNT_BATCH = 8;               // the resolve macros below are written for exactly 8

// ---- one batch of a bucket's records.  The records [r0, r1) of a bucket are read as aligned 16-byte pairs (pair q = records
// 2q and 2q + 1 of the buffer), CNT_BATCH / 2 pairs per lane and batch, all loads in flight together.
struct PairRange {
    const ulonglong2 *rec2;
    int64_t q0, q1, r0, r1;
    __device__ __forceinline__ PairRange(const uint64_t *rec, int64_t r0_, int64_t r1_)
        : rec2(reinterpret_cast<const ulonglong2 *>(rec)), q0(r0_ >> 1), q1((r1_ + 1) >> 1), r0(r0_), r1(r1_) {}
    static constexpr int64_t stride = (int64_t)BIG_BLOCK * (CNT_BATCH / 2);
    // pairs of the batch at `base`; lanes beyond the range get `pad` in both halves
    __device__ __forceinline__ void load(int64_t base, ulonglong2 (&v)[CNT_BATCH / 2], unsigned long long pad) const
    {
#pragma unroll
        for (int j = 0; j < CNT_BATCH / 2; ++j) {
            const int64_t q = base + (int64_t)j * BIG_BLOCK + threadIdx.x;
            v[j] = q < q1 ? rec2[q] : make_ulonglong2(pad, pad);
        }
    }
    // the NEXT batch's loads, issued behind the point where `dep` (something computed from the current batch) is known: without
    // the dependency the compiler hoists these conditional loads in front of the s_waitcnt vmcnt(0) for the current batch, which
    // then waits for them too -- the prefetch is gone, and a kernel that runs one workgroup per CU has nothing else to do meanwhile
    __device__ __forceinline__ void load_next(int64_t base, ulonglong2 (&v)[CNT_BATCH / 2], unsigned long long pad, uint32_t dep) const
    {
        int64_t b = base + stride;
        asm volatile("" : "+v"(b) : "v"(dep));
        load(b, v, pad);
    }
    // which of the batch's records belong to the bucket (the first / last pair may straddle its ends)
    __device__ __forceinline__ void live(int64_t base, bool (&l)[CNT_BATCH]) const
    {
#pragma unroll
        for (int j = 0; j < CNT_BATCH / 2; ++j) {
            const int64_t q = base + (int64_t)j * BIG_BLOCK + threadIdx.x;
            l[2 * j] = q < q1 && 2 * q >= r0;
            l[2 * j + 1] = q < q1 && 2 * q + 1 < r1;
        }
    }
};

__global__ __launch_bounds__(BIG_BLOCK) void bucket_count_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                 HashView t, int accumulate, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (r0 == r1 && accumulate) return;                         // nothing to add, slice stays as it is
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) tab[i] = accumulate ? slice[i] : 0ull;
    __syncthreads();
    bool full = false;
    const PairRange pr(rec, r0, r1);
    ulonglong2 nxt[CNT_BATCH / 2];
    pr.load(pr.q0, nxt, 0ull);
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {
        uint64_t rr[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.live(base, live);
#pragma unroll
        for (int j = 0; j < CNT_BATCH / 2; ++j) {
            rr[2 * j] = live[2 * j] ? nxt[j].x & REC_KEY_MASK : 0ull;
            rr[2 * j + 1] = live[2 * j + 1] ? nxt[j].y & REC_KEY_MASK : 0ull;
        }
        pr.load(base + PairRange::stride, nxt, 0ull);               // software pipeline: the next batch's loads fly during the inserts
        uint32_t ss[CNT_BATCH];
        unsigned long long first[CNT_BATCH];
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) {
            ss[j] = (uint32_t)(rr[j] >> hsh) & smask;
            first[j] = live[j] ? tab[ss[j]] : 0ull;
        }
        // resolved one by one, written out by hand: an unrolled loop around the probe loop is not unrolled by hipcc and
        // would push the batch arrays into scratch
#define PG_RESOLVE(J) full |= !lds_insert(tab, smask, limit, rr[J], live[J], ss[J], first[J]);
        PG_RESOLVE(0) PG_RESOLVE(1) PG_RESOLVE(2) PG_RESOLVE(3) PG_RESOLVE(4) PG_RESOLVE(5) PG_RESOLVE(6) PG_RESOLVE(7)
#undef PG_RESOLVE
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) slice[i] = tab[i];
}

// split-table view of a batch: tag (the key's bits below the bucket / group id, | 0x80000000), home slot, row id
__device__ __forceinline__ void split32(const ulonglong2 (&v)[CNT_BATCH / 2], uint32_t tag_mask, int hsh, uint32_t smask,
                                        uint32_t (&tg)[CNT_BATCH], uint32_t (&ss)[CNT_BATCH], uint32_t (&row)[CNT_BATCH])
{
#pragma unroll
    for (int j = 0; j < CNT_BATCH / 2; ++j) {
        const uint64_t k0 = v[j].x & REC_KEY_MASK, k1 = v[j].y & REC_KEY_MASK;
        tg[2 * j] = ((uint32_t)k0 & tag_mask) | 0x80000000u;
        tg[2 * j + 1] = ((uint32_t)k1 & tag_mask) | 0x80000000u;
        ss[2 * j] = (uint32_t)(k0 >> hsh) & smask;
        ss[2 * j + 1] = (uint32_t)(k1 >> hsh) & smask;
        row[2 * j] = (uint32_t)(v[j].x >> REC_KEY_BITS);
        row[2 * j + 1] = (uint32_t)(v[j].y >> REC_KEY_BITS);
    }
}

// the two 4-byte planes of a slice <-> its packed 8-byte slots (counts are clamped to the saturation value on the way out)
__device__ __forceinline__ void planes_from_slice(uint32_t *tags, uint32_t *cnts, uint32_t n_slots, uint32_t tag_mask, const uint64_t *slice)
{
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) {
        const uint64_t v = slice ? slice[i] : 0ull;
        tags[i] = v ? ((uint32_t)(v >> HASH_CBITS) & tag_mask) | 0x80000000u : 0u;
        cnts[i] = (uint32_t)(v & HASH_CMASK);
    }
}
__device__ __forceinline__ uint64_t packed_slot(uint64_t high, uint32_t tag, uint32_t tag_mask, uint32_t count)
{
    return ((high | (tag & tag_mask)) << HASH_CBITS) | (count < HASH_SAT ? count : HASH_SAT);
}
__device__ __forceinline__ void slice_from_planes(const uint32_t *tags, const uint32_t *cnts, uint32_t n_slots, uint32_t tag_mask, uint64_t high,
                                                  uint64_t *slice)
{
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) slice[i] = tags[i] ? packed_slot(high, tags[i], tag_mask, cnts[i]) : 0ull;
}

// B with a split LDS table (buckets >= 2^11, i.e. the key's bits below the bucket id fit 31 bits): tags[] = those bits
// | 0x80000000, counts[] = plain uint32 -- the same 128 KiB, but every LDS operation is 4 bytes wide and the increment is a
// 32-bit add with no saturation test (a bucket has < 2^32 records; counts are clamped to SAT when the slots are packed).
__device__ __forceinline__ bool lds_insert32(uint32_t *tags, uint32_t *cnts, uint32_t smask, uint32_t limit, uint32_t tag, bool live,
                                             uint32_t s, uint32_t cur)
{
    if (!live) return true;
    for (uint32_t i = 0; i < limit; ++i) {
        if (cur == 0) {
            cur = atomicCAS(&tags[s], 0u, tag);
            if (cur == 0) cur = tag;
        }
        if (cur == tag) { atomicAdd(&cnts[s], 1u); return true; }
        s = (s + 1) & smask;
        cur = tags[s];
    }
    return false;
}

__global__ __launch_bounds__(BIG_BLOCK) void bucket_count32_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                   HashView t, int accumulate, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    uint32_t *tags = reinterpret_cast<uint32_t *>(tab), *cnts = tags + n_slots;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const int tag_bits = KEY_BITS - (t.log2_slots - t.log2_bucket);  // <= 31
    const uint32_t tag_mask = (1u << tag_bits) - 1u;
    uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (r0 == r1 && accumulate) return;
    planes_from_slice(tags, cnts, n_slots, tag_mask, accumulate ? slice : nullptr);
    __syncthreads();
    bool full = false;
    const PairRange pr(rec, r0, r1);
    ulonglong2 nxt[CNT_BATCH / 2];
    pr.load(pr.q0, nxt, 0ull);
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {
        uint32_t tg[CNT_BATCH], ss[CNT_BATCH], row[CNT_BATCH], first[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.live(base, live);
        split32(nxt, tag_mask, hsh, smask, tg, ss, row);
        pr.load_next(base, nxt, 0ull, tg[0]);                       // software pipeline: the next batch's loads fly during the inserts
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) first[j] = live[j] ? tags[ss[j]] : 0u;
#define PG_RESOLVE(J) full |= !lds_insert32(tags, cnts, smask, limit, tg[J], live[J], ss[J], first[J]);
        PG_RESOLVE(0) PG_RESOLVE(1) PG_RESOLVE(2) PG_RESOLVE(3) PG_RESOLVE(4) PG_RESOLVE(5) PG_RESOLVE(6) PG_RESOLVE(7)
#undef PG_RESOLVE
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    slice_from_planes(tags, cnts, n_slots, tag_mask, (uint64_t)blockIdx.x << tag_bits, slice);     // the bucket id is the key's top bits
}

// B for the multi-GPU path: the rank's table is never materialised.  The table descriptor has the geometry of the UNION
// over all ranks (so that the records are partitioned the way the final lookups need them), but one rank's share of the
// keys is 2^g times sparser: a workgroup therefore counts 2^g adjacent final buckets together in one LDS table of the
// usual size (hash bits after the group's), and instead of a 2^log2_bucket-slot image per final bucket it writes only
// the occupied entries, split by final bucket, to scratch[off[b] ..] (a bucket has no more distinct keys than records)
// and their number to fill[b] -- exactly what the exchange sends.  The LDS rebuild after the all-gather writes the table.
__global__ __launch_bounds__(BIG_BLOCK) void bucket_count_compact_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                         HashView t, int g, uint64_t *__restrict__ scratch,
                                                                         long long *__restrict__ fill, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ uint32_t qcnt[1 << PG_DEFERRED_MAX_GROUP_LOG2];
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - (t.log2_slots - g);                  // slot inside the group's table
    const int bsh = KEY_BITS - (t.log2_slots - t.log2_bucket);      // final bucket id
    const uint32_t qmask = (1u << g) - 1u;
    const int64_t b0 = (int64_t)blockIdx.x << g;
    const int64_t r0 = (int64_t)off[b0], r1 = (int64_t)off[b0 + (1 << g)];
    if (threadIdx.x <= qmask) qcnt[threadIdx.x] = 0;
    if (r0 == r1) { if (threadIdx.x <= qmask) fill[b0 + threadIdx.x] = 0; return; }
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) tab[i] = 0ull;
    __syncthreads();
    bool full = false;
    const PairRange pr(rec, r0, r1);
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {
        ulonglong2 v[CNT_BATCH / 2];
        uint64_t rr[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.load(base, v, 0ull);
        pr.live(base, live);
#pragma unroll
        for (int j = 0; j < CNT_BATCH / 2; ++j) {
            rr[2 * j] = live[2 * j] ? v[j].x & REC_KEY_MASK : 0ull;
            rr[2 * j + 1] = live[2 * j + 1] ? v[j].y & REC_KEY_MASK : 0ull;
        }
        uint32_t ss[CNT_BATCH];
        unsigned long long first[CNT_BATCH];
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) {
            ss[j] = (uint32_t)(rr[j] >> hsh) & smask;
            first[j] = live[j] ? tab[ss[j]] : 0ull;
        }
#define PG_RESOLVE(J) full |= !lds_insert(tab, smask, limit, rr[J], live[J], ss[J], first[J]);
        PG_RESOLVE(0) PG_RESOLVE(1) PG_RESOLVE(2) PG_RESOLVE(3) PG_RESOLVE(4) PG_RESOLVE(5) PG_RESOLVE(6) PG_RESOLVE(7)
#undef PG_RESOLVE
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) {
        const unsigned long long v = tab[i];
        if (v) {
            const uint32_t q = (uint32_t)((v >> HASH_CBITS) >> bsh) & qmask;
            scratch[off[b0 + q] + atomicAdd(&qcnt[q], 1u)] = v;
        }
    }
    __syncthreads();
    if (threadIdx.x <= qmask) fill[b0 + threadIdx.x] = (long long)qcnt[threadIdx.x];
}

// the same with the split 32-bit LDS table (the key's bits below the GROUP id fit 31 bits)
__global__ __launch_bounds__(BIG_BLOCK) void bucket_count_compact32_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                           HashView t, int g, uint64_t *__restrict__ scratch,
                                                                           long long *__restrict__ fill, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ uint32_t qcnt[1 << PG_DEFERRED_MAX_GROUP_LOG2];
    const uint32_t n_slots = 1u << t.log2_bucket;
    uint32_t *tags = reinterpret_cast<uint32_t *>(tab), *cnts = tags + n_slots;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - (t.log2_slots - g);                  // slot inside the group's table
    const int tag_bits = KEY_BITS - (t.log2_slots - t.log2_bucket - g);   // key bits below the group id, <= 31
    const uint32_t tag_mask = (1u << tag_bits) - 1u;
    const uint32_t qmask = (1u << g) - 1u;
    const int64_t b0 = (int64_t)blockIdx.x << g;
    const int64_t r0 = (int64_t)off[b0], r1 = (int64_t)off[b0 + (1 << g)];
    if (threadIdx.x <= qmask) qcnt[threadIdx.x] = 0;
    if (r0 == r1) { if (threadIdx.x <= qmask) fill[b0 + threadIdx.x] = 0; return; }
    planes_from_slice(tags, cnts, n_slots, tag_mask, nullptr);
    __syncthreads();
    bool full = false;
    const PairRange pr(rec, r0, r1);
    ulonglong2 v[CNT_BATCH / 2];
    pr.load(pr.q0, v, 0ull);
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {
        uint32_t tg[CNT_BATCH], ss[CNT_BATCH], row[CNT_BATCH], first[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.live(base, live);
        split32(v, tag_mask, hsh, smask, tg, ss, row);
        pr.load_next(base, v, 0ull, tg[0]);                         // the next batch's loads fly during the inserts
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) first[j] = live[j] ? tags[ss[j]] : 0u;
#define PG_RESOLVE(J) full |= !lds_insert32(tags, cnts, smask, limit, tg[J], live[J], ss[J], first[J]);
        PG_RESOLVE(0) PG_RESOLVE(1) PG_RESOLVE(2) PG_RESOLVE(3) PG_RESOLVE(4) PG_RESOLVE(5) PG_RESOLVE(6) PG_RESOLVE(7)
#undef PG_RESOLVE
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    const uint64_t high = (uint64_t)blockIdx.x << tag_bits;         // the group id is the key's top bits
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) {
        const uint32_t tg = tags[i];
        if (tg) {
            const uint32_t q = ((tg & tag_mask) >> (tag_bits - g)) & qmask;          // the final bucket inside the group
            scratch[off[b0 + q] + atomicAdd(&qcnt[q], 1u)] = packed_slot(high, tg, tag_mask, cnts[i]);
        }
    }
    __syncthreads();
    if (threadIdx.x <= qmask) fill[b0 + threadIdx.x] = (long long)qcnt[threadIdx.x];
}

// the deferred entries of bucket b, scratch[off[b] .. off[b] + fill[b]), to out[seg[b] ..]: one wavefront per bucket
__global__ __launch_bounds__(BLOCK) void deferred_gather_kernel(const uint64_t *__restrict__ scratch, const unsigned long long *__restrict__ off,
                                                                const long long *__restrict__ fill, const long long *__restrict__ seg,
                                                                int64_t n_buckets, uint64_t *__restrict__ out)
{
    const int64_t b = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= n_buckets) return;
    const uint64_t *src = scratch + off[b];
    uint64_t *dst = out + seg[b];
    const long long n = fill[b];
    for (long long i = threadIdx.x & 63; i < n; i += 64) dst[i] = src[i];
}

constexpr int MERGE_BATCH = 4;             // entries per lane in flight in the merge kernels

// The exchange format: 6 bytes per entry instead of 8.  Inside bucket b a key is its bits below the bucket id (the tag, <= 31
// bits for >= 2^11 buckets) and a count is almost always < 2^16, so an entry travels as a 4-byte tag and a 2-byte count in
// two planes; a count >= 0xffff sends 0xffff there and the remainder as a full 8-byte entry in a (tiny) overflow list that
// is merged afterwards -- sums are exact.  tag_elem[b] / cnt_elem[b]: where bucket b's first tag / count goes, in elements
// of the uint32 / uint16 view of the send buffer.
__global__ __launch_bounds__(BLOCK) void deferred_gather_planes_kernel(const uint64_t *__restrict__ scratch, const unsigned long long *__restrict__ off,
                                                                       const long long *__restrict__ fill, const long long *__restrict__ tag_elem,
                                                                       const long long *__restrict__ cnt_elem, int64_t n_buckets, uint32_t tag_mask,
                                                                       uint32_t *__restrict__ out32, uint16_t *__restrict__ out16,
                                                                       uint64_t *__restrict__ ovf, unsigned long long *__restrict__ ovf_count,
                                                                       unsigned long long ovf_cap, uint32_t *status)
{
    const int64_t b = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (b >= n_buckets) return;
    const uint64_t *src = scratch + off[b];
    uint32_t *t32 = out32 + tag_elem[b];
    uint16_t *c16 = out16 + cnt_elem[b];
    const long long n = fill[b];
    for (long long i = threadIdx.x & 63; i < n; i += 64) {
        const uint64_t e = src[i];
        const uint32_t c = (uint32_t)(e & HASH_CMASK);
        t32[i] = (uint32_t)(e >> HASH_CBITS) & tag_mask;
        c16[i] = (uint16_t)(c < 0xffffu ? c : 0xffffu);
        if (c >= 0xffffu && c > 0xffffu) {                          // the remainder travels as a whole entry
            const unsigned long long at = atomicAdd(ovf_count, 1ull);
            if (at < ovf_cap) ovf[at] = (e & ~HASH_CMASK) | (uint64_t)(c - 0xffffu);
            else atomicOr(status, 2u);
        }
    }
}

// rebuild of buckets [bucket_base, bucket_base + gridDim.x) from the gathered planes of n_parts ranks: part p's tags are at
// buf + p * part_stride, its counts `cap` tags later; seg[p][j] = index of the first entry of bucket bucket_base + j
__global__ __launch_bounds__(BIG_BLOCK) void bucket_merge_planes_kernel(const uint8_t *__restrict__ buf, int64_t part_stride, int64_t cap,
                                                                        const long long *__restrict__ seg, int n_parts, HashView t,
                                                                        uint32_t *status, int64_t bucket_base, int64_t n_seg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    uint32_t *tags = reinterpret_cast<uint32_t *>(tab), *cnts = tags + n_slots;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const int tag_bits = KEY_BITS - (t.log2_slots - t.log2_bucket);
    const uint32_t tag_mask = (1u << tag_bits) - 1u;
    const int64_t bucket = bucket_base + blockIdx.x;
    uint64_t *slice = t.slots + ((uint64_t)bucket << t.log2_bucket);
    planes_from_slice(tags, cnts, n_slots, tag_mask, nullptr);
    __syncthreads();
    bool full = false;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t a = seg[p * (n_seg + 1) + blockIdx.x], b = seg[p * (n_seg + 1) + blockIdx.x + 1];
        const uint32_t *pt = reinterpret_cast<const uint32_t *>(buf + p * part_stride);
        const uint16_t *pc = reinterpret_cast<const uint16_t *>(buf + p * part_stride + 4 * cap);
        for (int64_t base = a; base < b; base += (int64_t)BIG_BLOCK * MERGE_BATCH) {
            uint32_t tg[MERGE_BATCH], add[MERGE_BATCH], ss[MERGE_BATCH], first[MERGE_BATCH];
            bool live[MERGE_BATCH];
#pragma unroll
            for (int j = 0; j < MERGE_BATCH; ++j) {
                const int64_t i = base + (int64_t)j * BIG_BLOCK + threadIdx.x;
                live[j] = i < b;
                tg[j] = live[j] ? pt[i] : 0u;
                add[j] = live[j] ? (uint32_t)pc[i] : 0u;
            }
#pragma unroll
            for (int j = 0; j < MERGE_BATCH; ++j) {
                ss[j] = (tg[j] >> hsh) & smask;                     // the slot index is the top bits of the tag
                tg[j] = (tg[j] & tag_mask) | 0x80000000u;
                first[j] = live[j] ? tags[ss[j]] : 0u;
            }
#define PG_MERGE(J)                                                                                                         \
            if (live[J]) {                                                                                                  \
                uint32_t sl = ss[J], cur = first[J];                                                                        \
                bool done = false;                                                                                          \
                for (uint32_t tries = 0; tries < limit && !done; ++tries) {                                                 \
                    if (cur == 0) { cur = atomicCAS(&tags[sl], 0u, tg[J]); if (cur == 0) cur = tg[J]; }                     \
                    if (cur == tg[J]) { atomicAdd(&cnts[sl], add[J]); done = true; }                                        \
                    else { sl = (sl + 1) & smask; cur = tags[sl]; }                                                         \
                }                                                                                                           \
                full |= !done;                                                                                              \
            }
            PG_MERGE(0) PG_MERGE(1) PG_MERGE(2) PG_MERGE(3)
#undef PG_MERGE
        }
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    slice_from_planes(tags, cnts, n_slots, tag_mask, (uint64_t)bucket << tag_bits, slice);
}

// Bucket-wise merge of other tables into this one: the compacted tables of the other ranks arrive bucket by bucket
// (a table's slots are laid out by bucket, so compaction keeps bucket order).  One workgroup per bucket loads its slice
// into LDS, adds every foreign entry of that bucket (counts saturate exactly) and writes the slice back.
//   pairs  : the foreign tables' occupied slots, concatenated part after part
//   seg    : [n_parts][n_buckets + 1] offsets into `pairs` (absolute)
// rebuild != 0: the slice is built from the parts alone (they include this rank's own compacted table), so the old
// slice is neither read nor assumed to be initialised.
__device__ __forceinline__ bool lds_merge(unsigned long long *tab, uint32_t smask, uint32_t limit, uint64_t code, uint32_t add,
                                          uint32_t s, unsigned long long cur)
{
    for (uint32_t tries = 0; tries < limit; ++tries) {
        for (;;) {
            if (cur != 0 && (cur >> HASH_CBITS) != code) break;
            const uint32_t have = (uint32_t)(cur & HASH_CMASK);
            const uint32_t sum = have + add > HASH_SAT ? HASH_SAT : have + add;
            const unsigned long long old = atomicCAS(&tab[s], cur, (unsigned long long)((code << HASH_CBITS) | sum));
            if (old == cur) return true;
            cur = old;
        }
        s = (s + 1) & smask;
        cur = tab[s];
    }
    return false;
}

// one foreign slot `e` (slot format, 0 = nothing) into the LDS table, its first probe (`first` = tab[s]) already fetched: the
// inner step of bucket_merge_kernel and table_merge_aligned_kernel.  false = the bucket has no room for it.
__device__ __forceinline__ bool lds_merge_entry(unsigned long long *tab, uint32_t smask, uint32_t limit, uint64_t e, uint32_t s,
                                                unsigned long long first)
{
    if (e == 0) return true;
    uint32_t add = (uint32_t)(e & HASH_CMASK);
    if (add > HASH_SAT) add = HASH_SAT;
    return lds_merge(tab, smask, limit, e >> HASH_CBITS, add, s, first);
}

// The launch covers buckets [bucket_base, bucket_base + gridDim.x); seg has n_seg + 1 entries per part, entry j for
// bucket bucket_base + j (a whole-table launch: base 0, n_seg = number of buckets).
__global__ __launch_bounds__(BIG_BLOCK) void bucket_merge_kernel(const uint64_t *__restrict__ pairs, const long long *__restrict__ seg,
                                                                 int n_parts, HashView t, uint32_t *status, int rebuild,
                                                                 int64_t bucket_base, int64_t n_seg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const int64_t n_buckets = n_seg;                                // row stride of seg is n_seg + 1
    uint64_t *slice = t.slots + ((uint64_t)(bucket_base + blockIdx.x) << t.log2_bucket);
    int64_t total = 0;
    for (int p = 0; p < n_parts; ++p) total += seg[p * (n_buckets + 1) + blockIdx.x + 1] - seg[p * (n_buckets + 1) + blockIdx.x];
    if (total == 0 && !rebuild) return;
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) tab[i] = rebuild ? 0ull : slice[i];
    __syncthreads();
    bool full = false;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t a = seg[p * (n_buckets + 1) + blockIdx.x], b = seg[p * (n_buckets + 1) + blockIdx.x + 1];
        for (int64_t base = a; base < b; base += (int64_t)BIG_BLOCK * MERGE_BATCH) {
            uint64_t e[MERGE_BATCH];
#pragma unroll
            for (int j = 0; j < MERGE_BATCH; ++j) {                  // a part's whole segment of this bucket is usually one batch
                const int64_t i = base + (int64_t)j * BIG_BLOCK + threadIdx.x;
                e[j] = i < b ? pairs[i] : 0ull;
            }
            uint32_t ss[MERGE_BATCH];
            unsigned long long first[MERGE_BATCH];
#pragma unroll
            for (int j = 0; j < MERGE_BATCH; ++j) {
                ss[j] = (uint32_t)((e[j] >> HASH_CBITS) >> hsh) & smask;
                first[j] = e[j] ? tab[ss[j]] : 0ull;
            }
#define PG_MERGE(J) full |= !lds_merge_entry(tab, smask, limit, e[J], ss[J], first[J]);
            PG_MERGE(0) PG_MERGE(1) PG_MERGE(2) PG_MERGE(3)
#undef PG_MERGE
        }
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) slice[i] = tab[i];
}

// the merge / rebuild with the split 32-bit LDS table: an entry adds its count with ONE 32-bit LDS add (no CAS loop; the sum
// of all parts' counts stays far below 2^32 and is clamped to SAT when the slots are packed -- the exact saturating sum)
__global__ __launch_bounds__(BIG_BLOCK) void bucket_merge32_kernel(const uint64_t *__restrict__ pairs, const long long *__restrict__ seg,
                                                                   int n_parts, HashView t, uint32_t *status, int rebuild,
                                                                   int64_t bucket_base, int64_t n_seg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket;
    uint32_t *tags = reinterpret_cast<uint32_t *>(tab), *cnts = tags + n_slots;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const int tag_bits = KEY_BITS - (t.log2_slots - t.log2_bucket);
    const uint32_t tag_mask = (1u << tag_bits) - 1u;
    const int64_t bucket = bucket_base + blockIdx.x;
    uint64_t *slice = t.slots + ((uint64_t)bucket << t.log2_bucket);
    int64_t total = 0;
    for (int p = 0; p < n_parts; ++p) total += seg[p * (n_seg + 1) + blockIdx.x + 1] - seg[p * (n_seg + 1) + blockIdx.x];
    if (total == 0 && !rebuild) return;
    planes_from_slice(tags, cnts, n_slots, tag_mask, rebuild ? nullptr : slice);
    __syncthreads();
    bool full = false;
    for (int p = 0; p < n_parts; ++p) {
        const int64_t a = seg[p * (n_seg + 1) + blockIdx.x], b = seg[p * (n_seg + 1) + blockIdx.x + 1];
        for (int64_t base = a; base < b; base += (int64_t)BIG_BLOCK * MERGE_BATCH) {
            uint64_t e[MERGE_BATCH];
#pragma unroll
            for (int j = 0; j < MERGE_BATCH; ++j) {
                const int64_t i = base + (int64_t)j * BIG_BLOCK + threadIdx.x;
                e[j] = i < b ? pairs[i] : 0ull;
            }
            uint32_t ss[MERGE_BATCH], first[MERGE_BATCH];
#pragma unroll
            for (int j = 0; j < MERGE_BATCH; ++j) {
                ss[j] = (uint32_t)((e[j] >> HASH_CBITS) >> hsh) & smask;
                first[j] = e[j] ? tags[ss[j]] : 0u;
            }
#define PG_MERGE(J)                                                                                                         \
            if (e[J]) {                                                                                                     \
                const uint32_t tg = ((uint32_t)(e[J] >> HASH_CBITS) & tag_mask) | 0x80000000u;                              \
                uint32_t add = (uint32_t)(e[J] & HASH_CMASK);                                                               \
                if (add > HASH_SAT) add = HASH_SAT;                                                                         \
                uint32_t sl = ss[J], cur = first[J];                                                                        \
                bool done = false;                                                                                          \
                for (uint32_t tries = 0; tries < limit && !done; ++tries) {                                                 \
                    if (cur == 0) { cur = atomicCAS(&tags[sl], 0u, tg); if (cur == 0) cur = tg; }                           \
                    if (cur == tg) { atomicAdd(&cnts[sl], add); done = true; }                                              \
                    else { sl = (sl + 1) & smask; cur = tags[sl]; }                                                         \
                }                                                                                                           \
                full |= !done;                                                                                              \
            }
            PG_MERGE(0) PG_MERGE(1) PG_MERGE(2) PG_MERGE(3)
#undef PG_MERGE
        }
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    slice_from_planes(tags, cnts, n_slots, tag_mask, (uint64_t)bucket << tag_bits, slice);
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
constexpr int ALIGNED_PAIRS = 4;           // the resolve macro below is written for exactly 2 * 4 slots
struct MergeSources {
    const ulonglong2 *p[ALIGNED_MAX_SRCS];
};

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
    for (int p = 0; p < n_srcs; ++p) {
        const ulonglong2 *__restrict__ src = srcs.p[p] + first_pair;
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
                const uint64_t code = e[j] >> HASH_CBITS;                        // (hash: the key; mini: the code itself)
                ss[j] = (MINI ? mini_slot_hash<true>(code) : (uint32_t)(code >> hsh)) & smask;
                first[j] = e[j] ? tab[ss[j]] : 0ull;
            }
#define PG_MERGE(J) full |= !lds_merge_entry(tab, smask, limit, e[J], ss[J], first[J]);
            PG_MERGE(0) PG_MERGE(1) PG_MERGE(2) PG_MERGE(3) PG_MERGE(4) PG_MERGE(5) PG_MERGE(6) PG_MERGE(7)
#undef PG_MERGE
        }
    }
    if (full) atomicOr(status, PG_STATUS_TABLE_FULL);
    __syncthreads();
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>(t.slots) + first_pair;
    for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) out[i] = tab2[i];
}

// GENERAL (table_merge_kernel): any source kind into any destination kind, whatever the geometries.  The source's storage is
// streamed with the dump kernels' 16-byte loads (dump_load: four dense counters, four packed slots, or four keys with their four
// counts), MERGE_QUADS of them in flight per lane; an entry's code is the index (dense), key42_inverse of the key (hash), the
// slot's high bits (mini), key - 1 (planes).  It is ADDED to what the destination holds: atomicAdd (dense), the saturating
// compare-and-swap of kmer_merge_kernel placed by key42 + home_key / home_mini (hash / mini; the first probes of a lane's batch
// are issued before any is resolved, as table_query_kernel does), wide_add (wide / miniw: 32-bit sums).  A packed source's
// saturated count travels as the value it stores; a count that enters a packed table is clamped to HASH_COUNT_SAT first.
constexpr int MERGE_QUADS = 2;

// `add` more of `key` into a packed table, the sum stopping at HASH_COUNT_SAT exactly; s / cur = home slot and what a plain load
// found there (stale at worst: the compare-and-swap then returns the slot's real content)
__device__ __forceinline__ void hash_merge_from(const HashView &t, uint64_t s, uint64_t cur, uint64_t key, uint32_t add, uint32_t *status)
{
    const uint32_t limit = t.limit();
    for (uint32_t tries = 0; tries < limit; ++tries) {
        for (;;) {
            if (cur != 0 && (cur >> HASH_CBITS) != key) break;                   // occupied by another key
            const uint32_t have = (uint32_t)(cur & HASH_CMASK);
            const uint32_t sum = have + add > HASH_SAT ? HASH_SAT : have + add;
            const uint64_t old = atomicCAS((unsigned long long *)&t.slots[s], (unsigned long long)cur, (unsigned long long)((key << HASH_CBITS) | sum));
            if (old == cur) return;
            cur = old;
        }
        s = t.next(s);
        cur = __hip_atomic_load(&t.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    atomicOr(status, PG_STATUS_TABLE_FULL);
}

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
                code[i] = FORM == DUMP_HASH ? key42_inverse(raw[j]) : raw[j];
                key[i] = TK != TK_HASH ? code[i] : FORM == DUMP_HASH ? raw[j] : key42(code[i]);
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
#define PG_HOME(CODE) ((MINI ? mini_slot_hash<true>(CODE) : (uint32_t)((CODE) >> hsh)) & smask)
    if (op == COMBINE_MAX) {
        for (uint32_t i = threadIdx.x; i < n_pairs; i += BIG_BLOCK) tab2[i] = make_ulonglong2(0ull, 0ull);
        __syncthreads();
        bool full = false;
        for (int p = 0; p < 2; ++p) {
            const ulonglong2 *__restrict__ src = p ? b : a;
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
                    ss[j] = PG_HOME(e[j] >> HASH_CBITS);
                    first[j] = e[j] ? tab[ss[j]] : 0ull;
                }
#pragma unroll
                for (int j = 0; j < 2 * ALIGNED_PAIRS; ++j)
                    if (e[j] & HASH_CMASK) full |= !lds_larger(tab, smask, limit, e[j], ss[j], first[j]);
            }
        }
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
            for (uint32_t base = 0; base < n_pairs; base += BIG_BLOCK * ALIGNED_PAIRS) {
                uint64_t e[2 * ALIGNED_PAIRS];
#pragma unroll
                for (int j = 0; j < ALIGNED_PAIRS; ++j) {
                    const uint32_t i = base + (uint32_t)j * BIG_BLOCK + threadIdx.x;
                    const ulonglong2 v = i < n_pairs ? b[i] : make_ulonglong2(0ull, 0ull);
                    e[2 * j] = v.x;
                    e[2 * j + 1] = v.y;
                }
#pragma unroll
                for (int j = 0; j < 2 * ALIGNED_PAIRS; ++j) {
                    const uint32_t cb = (uint32_t)(e[j] & HASH_CMASK);
                    if (cb == 0) continue;                                       // (an empty slot; a stored count of 0 is b == 0)
                    const uint64_t code = e[j] >> HASH_CBITS;
                    uint32_t s = PG_HOME(code);
                    for (uint32_t tries = 0; tries < limit; ++tries) {
                        const unsigned long long cur = tab[s];
                        if (cur == 0) break;
                        if ((cur >> HASH_CBITS) == code) {
                            const uint32_t r = combine_result(op, (uint32_t)(cur & HASH_CMASK), cb);
                            if (r) tab[s] = (unsigned long long)((code << HASH_CBITS) | r);
                            if (op == COMBINE_MIN || op == COMBINE_LEFT || r == 0) atomicOr(&flags[s >> 5], 1u << (s & 31));
                            break;
                        }
                        s = (s + 1) & smask;
                    }
                }
            }
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
        const uint32_t s = PG_HOME(v[j] >> HASH_CBITS);
        lds_merge_entry(tab, smask, limit, v[j], s, tab[s]);                     // (always finds room: fewer entries than the bucket held)
    }
#undef PG_HOME
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
    uint64_t key[N], hh[N], cur[N];
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
            code[i] = FORM == DUMP_HASH ? key42_inverse(raw[j]) : raw[j];
            key[i] = hh[i] = cur[i] = 0;
            if (TK == TK_NONE || ca[i] == 0) continue;
            if (TK == TK_DENSE) {
                cur[i] = (code[i] >> (2 * k)) == 0 ? dense_b[(uint32_t)code[i]] : 0u;          // (never indexed beyond 4^k)
            } else {
                key[i] = TK != TK_HASH ? code[i] : FORM == DUMP_HASH ? raw[j] : key42(code[i]);
                hh[i] = TK == TK_WIDE ? b.home_wide(code[i]) : (TK == TK_MINI || TK == TK_MINIW) ? b.home_mini(code[i], k) : b.home_key(key[i]);
                cur[i] = b.slots[hh[i]];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        cb[i] = 0;
        if (TK == TK_NONE || ca[i] == 0) continue;
        bool found;
        if (TK == TK_DENSE) cb[i] = (uint32_t)cur[i];
        else if (TK == TK_WIDE || TK == TK_MINIW) cb[i] = wide_probe(b, hh[i], cur[i], key[i], &found);
        else cb[i] = hash_probe(b, hh[i], cur[i], key[i], &found);
    }
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

// occupied slots of every bucket: the segment lengths of a bucket-ordered compaction (one workgroup per bucket)
__global__ __launch_bounds__(BLOCK) void bucket_fill_kernel(const uint64_t *__restrict__ slots, int log2_bucket, long long *__restrict__ fill)
{
    __shared__ uint32_t part[WAVES];
    const ulonglong2 *s2 = reinterpret_cast<const ulonglong2 *>(slots + ((uint64_t)blockIdx.x << log2_bucket));
    const uint32_t n2 = 1u << (log2_bucket - 1);
    uint32_t c = 0;
    for (uint32_t i = threadIdx.x; i < n2; i += BLOCK) {
        const ulonglong2 v = s2[i];
        c += (v.x != 0) + (v.y != 0);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < WAVES; ++w) tot += part[w];
        fill[blockIdx.x] = (long long)tot;
    }
}

// bucket-ordered compaction: the occupied slots of bucket b go to out[seg[b] .. seg[b + 1]) (seg = exclusive scan of the
// fills; order inside a bucket is free, the merge inserts them one by one)
__global__ __launch_bounds__(BLOCK) void table_compact_kernel(const uint64_t *__restrict__ slots, int log2_bucket,
                                                              const long long *__restrict__ seg, uint64_t *__restrict__ out)
{
    __shared__ uint32_t cursor;
    if (threadIdx.x == 0) cursor = 0;
    __syncthreads();
    const uint64_t *slice = slots + ((uint64_t)blockIdx.x << log2_bucket);
    uint64_t *dst = out + seg[blockIdx.x];
    const uint32_t n = 1u << log2_bucket;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = 0; base < n; base += BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < n ? slice[i] : 0ull;
        const unsigned long long m = __ballot(v != 0);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t at = 0;
            if ((int)lane == leader) at = atomicAdd(&cursor, (uint32_t)__popcll(m));
            at = __shfl(at, leader);
            if (v != 0) dst[at + __popcll(m & ((1ull << lane) - 1ull))] = v;
        }
    }
}

// the occupied slots of the launch's buckets (slots points at the first of them) in the 6-byte exchange format: bucket j's
// tags from element tag_elem[j] of the uint32 view of the buffer, its counts from element cnt_elem[j] of the uint16 view;
// remainders of counts >= 0xffff go to the overflow list as whole entries
__global__ __launch_bounds__(BLOCK) void table_compact_planes_kernel(const uint64_t *__restrict__ slots, int log2_bucket,
                                                                     const long long *__restrict__ tag_elem, const long long *__restrict__ cnt_elem,
                                                                     uint32_t tag_mask, uint32_t *__restrict__ out32, uint16_t *__restrict__ out16,
                                                                     uint64_t *__restrict__ ovf, unsigned long long *__restrict__ ovf_count,
                                                                     unsigned long long ovf_cap, uint32_t *status)
{
    __shared__ uint32_t cursor;
    if (threadIdx.x == 0) cursor = 0;
    __syncthreads();
    const uint64_t *slice = slots + ((uint64_t)blockIdx.x << log2_bucket);
    uint32_t *t32 = out32 + tag_elem[blockIdx.x];
    uint16_t *c16 = out16 + cnt_elem[blockIdx.x];
    const uint32_t n = 1u << log2_bucket;
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t base = 0; base < n; base += BLOCK) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < n ? slice[i] : 0ull;
        const unsigned long long m = __ballot(v != 0);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t at = 0;
            if ((int)lane == leader) at = atomicAdd(&cursor, (uint32_t)__popcll(m));
            at = __shfl(at, leader);
            if (v != 0) {
                const uint32_t j = at + __popcll(m & ((1ull << lane) - 1ull));
                const uint32_t c = (uint32_t)(v & HASH_CMASK);
                t32[j] = (uint32_t)(v >> HASH_CBITS) & tag_mask;
                c16[j] = (uint16_t)(c < 0xffffu ? c : 0xffffu);
                if (c > 0xffffu) {
                    const unsigned long long o = atomicAdd(ovf_count, 1ull);
                    if (o < ovf_cap) ovf[o] = (v & ~HASH_CMASK) | (uint64_t)(c - 0xffffu);
                    else atomicOr(status, 2u);
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------- K3 by shuffle

// count of one record's code in the LDS copy of its bucket slice, starting from an already fetched first slot
__device__ __forceinline__ uint32_t lds_lookup(const unsigned long long *tab, uint32_t smask, uint32_t limit, uint64_t code,
                                               uint32_t s, unsigned long long cur, bool *found)
{
    for (uint32_t i = 0; i < limit; ++i) {
        if (cur == 0) break;
        if ((cur >> HASH_CBITS) == code) { *found = true; return (uint32_t)(cur & HASH_CMASK); }
        s = (s + 1) & smask;
        cur = tab[s];
    }
    *found = false;
    return 0;
}

// S1: one workgroup per bucket: the (final, possibly merged) slice is loaded into LDS and every record of the bucket
// that lies inside a row becomes the 32-bit word (row << vbits | count / window) if that bin is < vsize.  Words are
// packed at the front of the bucket's record range (order irrelevant); emit_end[b] = one past the last word.
__global__ __launch_bounds__(BIG_BLOCK) void bucket_lookup_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                  HashView t, uint32_t window, uint32_t vsize, int vbits,
                                                                  uint32_t *__restrict__ words, unsigned long long *__restrict__ emit_end)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ uint32_t emitted;
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (threadIdx.x == 0) emitted = 0;
    if (r0 == r1) { if (threadIdx.x == 0) emit_end[blockIdx.x] = (unsigned long long)r0; return; }
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) tab[i] = slice[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const PairRange pr(rec, r0, r1);
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {
        ulonglong2 v[CNT_BATCH / 2];
        uint64_t rr[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.load(base, v, ~0ull);                                    // a padding lane carries ROW_NONE
        pr.live(base, live);
#pragma unroll
        for (int j = 0; j < CNT_BATCH / 2; ++j) {
            rr[2 * j] = live[2 * j] ? v[j].x : ~0ull;
            rr[2 * j + 1] = live[2 * j + 1] ? v[j].y : ~0ull;
        }
        uint32_t ss[CNT_BATCH];
        unsigned long long first[CNT_BATCH];
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) {
            live[j] = live[j] && (uint32_t)(rr[j] >> REC_KEY_BITS) != ROW_NONE;
            ss[j] = (uint32_t)((rr[j] & REC_KEY_MASK) >> hsh) & smask;
            first[j] = live[j] ? tab[ss[j]] : 0ull;
        }
#define PG_EMIT(J)                                                                                                          \
        {                                                                                                                   \
            bool found = false;                                                                                             \
            uint32_t cnt = live[J] ? lds_lookup(tab, smask, limit, rr[J] & REC_KEY_MASK, ss[J], first[J], &found) : 0u;     \
            const uint32_t bin = cnt / window;                                                                              \
            const bool put = found && bin < vsize;                                                                          \
            const unsigned long long m = __ballot(put);                                                                     \
            if (m) {                                                                                                        \
                const int leader = __ffsll((long long)m) - 1;                                                               \
                uint32_t at = 0;                                                                                            \
                if ((int)lane == leader) at = atomicAdd(&emitted, (uint32_t)__popcll(m));                                   \
                at = __shfl(at, leader);                                                                                    \
                if (put) words[r0 + at + __popcll(m & ((1ull << lane) - 1ull))] = ((uint32_t)(rr[J] >> REC_KEY_BITS) << vbits) | bin; \
            }                                                                                                               \
        }
        PG_EMIT(0) PG_EMIT(1) PG_EMIT(2) PG_EMIT(3) PG_EMIT(4) PG_EMIT(5) PG_EMIT(6) PG_EMIT(7)
#undef PG_EMIT
    }
    __syncthreads();
    if (threadIdx.x == 0) emit_end[blockIdx.x] = (unsigned long long)r0 + emitted;
}

// S1 with a split LDS table (buckets >= 2^11): tags[] (the key's bits below the bucket id | 0x80000000) and, instead of the
// counts, bins[] = count / window computed ONCE per slot while the slice is loaded (0xffff: bin >= vsize, never emitted).
// A lookup is a 4-byte read and, on a hit, a 2-byte read; the division leaves the per-record path.
__global__ __launch_bounds__(BIG_BLOCK) void bucket_lookup32_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                    HashView t, uint32_t window, uint32_t vsize, int vbits,
                                                                    uint32_t *__restrict__ words, unsigned long long *__restrict__ emit_end)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ uint32_t emitted;
    const uint32_t n_slots = 1u << t.log2_bucket;
    uint32_t *tags = reinterpret_cast<uint32_t *>(tab);
    uint16_t *bins = reinterpret_cast<uint16_t *>(tags + n_slots);
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const int tag_bits = KEY_BITS - (t.log2_slots - t.log2_bucket);
    const uint32_t tag_mask = (1u << tag_bits) - 1u;
    const uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (threadIdx.x == 0) emitted = 0;
    if (r0 == r1) { if (threadIdx.x == 0) emit_end[blockIdx.x] = (unsigned long long)r0; return; }
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) {
        const uint64_t v = slice[i];
        const uint32_t bin = (uint32_t)(v & HASH_CMASK) / window;
        tags[i] = v ? ((uint32_t)(v >> HASH_CBITS) & tag_mask) | 0x80000000u : 0u;
        bins[i] = (uint16_t)(bin < vsize ? bin : 0xffffu);             // vsize <= PG_SHUFFLE_MAX_VSIZE = 512
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63;
    const PairRange pr(rec, r0, r1);
    ulonglong2 w[CNT_BATCH / 2];
    pr.load(pr.q0, w, ~0ull);                                       // a padding lane carries ROW_NONE
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {
        uint32_t tg[CNT_BATCH], ss[CNT_BATCH], first[CNT_BATCH], row[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.live(base, live);
        split32(w, tag_mask, hsh, smask, tg, ss, row);
        pr.load_next(base, w, ~0ull, tg[0]);
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) {
            live[j] = live[j] && row[j] != ROW_NONE;
            first[j] = live[j] ? tags[ss[j]] : 0u;
        }
#define PG_EMIT(J)                                                                                                          \
        {                                                                                                                   \
            uint32_t bin = 0xffffu;                                                                                         \
            if (live[J]) {                                                                                                  \
                uint32_t sl = ss[J], cur = first[J];                                                                        \
                for (uint32_t i = 0; i < limit && cur != 0; ++i) {                                                          \
                    if (cur == tg[J]) { bin = bins[sl]; break; }                                                            \
                    sl = (sl + 1) & smask;                                                                                  \
                    cur = tags[sl];                                                                                         \
                }                                                                                                           \
            }                                                                                                               \
            const bool put = bin != 0xffffu;                                                                                \
            const unsigned long long m = __ballot(put);                                                                     \
            if (m) {                                                                                                        \
                const int leader = __ffsll((long long)m) - 1;                                                               \
                uint32_t at = 0;                                                                                            \
                if ((int)lane == leader) at = atomicAdd(&emitted, (uint32_t)__popcll(m));                                   \
                at = __shfl(at, leader);                                                                                    \
                if (put) words[r0 + at + __popcll(m & ((1ull << lane) - 1ull))] = (row[J] << vbits) | bin;                  \
            }                                                                                                               \
        }
        PG_EMIT(0) PG_EMIT(1) PG_EMIT(2) PG_EMIT(3) PG_EMIT(4) PG_EMIT(5) PG_EMIT(6) PG_EMIT(7)
#undef PG_EMIT
    }
    __syncthreads();
    if (threadIdx.x == 0) emit_end[blockIdx.x] = (unsigned long long)r0 + emitted;
}

// B and S1 in one kernel (one GPU, a fresh table): while the bucket's counts are still in LDS -- right after the last insert --
// the bucket's records are streamed a second time (they were read a moment ago: L2 / MALL hits) and looked up, so the slice
// is never re-loaded or re-split, and the packed slice image is written out while the lookups run.
__global__ __launch_bounds__(BIG_BLOCK) void bucket_count_emit32_kernel(const uint64_t *__restrict__ rec, const unsigned long long *__restrict__ off,
                                                                        HashView t, uint32_t window, uint32_t vsize, int vbits,
                                                                        uint32_t *__restrict__ words, unsigned long long *__restrict__ emit_end,
                                                                        uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ uint32_t emitted;
    const uint32_t n_slots = 1u << t.log2_bucket;
    uint32_t *tags = reinterpret_cast<uint32_t *>(tab), *cnts = tags + n_slots;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = t.limit();
    const int hsh = KEY_BITS - t.log2_slots;
    const int tag_bits = KEY_BITS - (t.log2_slots - t.log2_bucket);
    const uint32_t tag_mask = (1u << tag_bits) - 1u;
    uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (threadIdx.x == 0) emitted = 0;
    planes_from_slice(tags, cnts, n_slots, tag_mask, nullptr);
    __syncthreads();
    bool full = false;
    const PairRange pr(rec, r0, r1);
    ulonglong2 v[CNT_BATCH / 2];
    pr.load(pr.q0, v, 0ull);
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {       // ---- count
        uint32_t tg[CNT_BATCH], ss[CNT_BATCH], row[CNT_BATCH], first[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.live(base, live);
        split32(v, tag_mask, hsh, smask, tg, ss, row);
        pr.load_next(base, v, 0ull, tg[0]);                         // the next batch's loads fly during the inserts
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) first[j] = live[j] ? tags[ss[j]] : 0u;
#define PG_RESOLVE(J) full |= !lds_insert32(tags, cnts, smask, limit, tg[J], live[J], ss[J], first[J]);
        PG_RESOLVE(0) PG_RESOLVE(1) PG_RESOLVE(2) PG_RESOLVE(3) PG_RESOLVE(4) PG_RESOLVE(5) PG_RESOLVE(6) PG_RESOLVE(7)
#undef PG_RESOLVE
    }
    if (full) atomicOr(status, 1u);
    __syncthreads();
    slice_from_planes(tags, cnts, n_slots, tag_mask, (uint64_t)blockIdx.x << tag_bits, slice);      // ---- the slice image (stores overlap the lookups)
    const uint32_t lane = threadIdx.x & 63;
    pr.load(pr.q0, v, ~0ull);                                       // a padding lane carries ROW_NONE
    for (int64_t base = pr.q0; base < pr.q1; base += PairRange::stride) {       // ---- lookups of the same records
        uint32_t tg[CNT_BATCH], ss[CNT_BATCH], first[CNT_BATCH], row[CNT_BATCH];
        bool live[CNT_BATCH];
        pr.live(base, live);
        split32(v, tag_mask, hsh, smask, tg, ss, row);
        pr.load_next(base, v, ~0ull, tg[0]);
#pragma unroll
        for (int j = 0; j < CNT_BATCH; ++j) {
            live[j] = live[j] && row[j] != ROW_NONE;
            first[j] = live[j] ? tags[ss[j]] : 0u;
        }
#define PG_EMIT(J)                                                                                                          \
        {                                                                                                                   \
            uint32_t bin = vsize;                                                                                           \
            if (live[J]) {                                                                                                  \
                uint32_t sl = ss[J], cur = first[J];                                                                        \
                for (uint32_t i = 0; i < limit && cur != 0; ++i) {                                                          \
                    if (cur == tg[J]) { bin = cnts[sl] / window; break; }                                                   \
                    sl = (sl + 1) & smask;                                                                                  \
                    cur = tags[sl];                                                                                         \
                }                                                                                                           \
            }                                                                                                               \
            const bool put = bin < vsize;                                                                                   \
            const unsigned long long m = __ballot(put);                                                                     \
            if (m) {                                                                                                        \
                const int leader = __ffsll((long long)m) - 1;                                                               \
                uint32_t at = 0;                                                                                            \
                if ((int)lane == leader) at = atomicAdd(&emitted, (uint32_t)__popcll(m));                                   \
                at = __shfl(at, leader);                                                                                    \
                if (put) words[r0 + at + __popcll(m & ((1ull << lane) - 1ull))] = (row[J] << vbits) | bin;                  \
            }                                                                                                               \
        }
        PG_EMIT(0) PG_EMIT(1) PG_EMIT(2) PG_EMIT(3) PG_EMIT(4) PG_EMIT(5) PG_EMIT(6) PG_EMIT(7)
#undef PG_EMIT
    }
    __syncthreads();
    if (threadIdx.x == 0) emit_end[blockIdx.x] = (unsigned long long)r0 + emitted;
}

// capacity of every row group (64 rows): the rows' character counts bound their k-mer counts
__global__ __launch_bounds__(BLOCK) void group_caps_kernel(const int64_t *__restrict__ row_start, const int64_t *__restrict__ row_end,
                                                           int64_t n_rows, int64_t n_groups_padded, unsigned long long *__restrict__ caps)
{
    const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (g >= n_groups_padded) return;
    unsigned long long c = 0;
    for (int64_t r = g << GROUP_ROWS_LOG2; r < ((g + 1) << GROUP_ROWS_LOG2) && r < n_rows; ++r) c += (unsigned long long)(row_end[r] - row_start[r]);
    caps[g] = c;
}

// S3: one workgroup per row group: LDS histogram [64 rows][vsize] of the group's (row, bin) words, written out as the
// rows of the abundance matrix (plain stores: every row belongs to exactly one group)
// WORD = uint16_t: the narrow words of a one-pass shuffle (row inside the group << vbits | bin; 0xffff = none)
// COUNTED (4-byte words): (n - 1) << PG_SHUFFLE_COUNT_SHIFT | row << vbits | bin stands for n equal words -- a lookup pass that
// merges the runs of a record itself (mini.hip) has left hardly any equal neighbours: no run detection here, the count is added
template <typename WORD, bool COUNTED = false>
__global__ __launch_bounds__(BIG_BLOCK) void row_hist_kernel(const WORD *__restrict__ words, const unsigned long long *__restrict__ goff,
                                                             const unsigned long long *__restrict__ gcnt, int vbits, uint32_t vsize,
                                                             int64_t n_rows, int32_t *__restrict__ abd_out, int64_t g0, int split)
{
    // split > 1: `split` workgroups share a group -- each takes a slice of its words and ADDS its partial histogram to rows that
    // were cleared beforehand.  For the groups of a last, mostly empty round of workgroups (one per CU: the histogram fills LDS):
    // 782 groups on 256 CUs are four rounds of which the last holds 14 groups.
    extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
    const int64_t g = g0 + (int64_t)(blockIdx.x / (unsigned)split);
    const int part = (int)(blockIdx.x % (unsigned)split);
    const int64_t row0 = g << GROUP_ROWS_LOG2;
    const int64_t rows_here = n_rows - row0 < (1 << GROUP_ROWS_LOG2) ? n_rows - row0 : (1 << GROUP_ROWS_LOG2);
    // rows lie `stride` words apart in LDS, an ODD number: with the matrix's own stride (V = 400 = 16 mod 32) the same bin of all
    // 64 rows falls on two of the 32 banks, and most k-mers of a sample share a handful of bins -- the adds were bank-conflict bound
    const uint32_t stride = vsize | 1u;
    const uint32_t n_bins = (uint32_t)rows_here * stride;
    for (uint32_t i = threadIdx.x; i < n_bins; i += BIG_BLOCK) hist[i] = 0;
    __syncthreads();
    int64_t a = (int64_t)goff[g], b = a + (int64_t)gcnt[g];
    if (split > 1) {
        const int64_t len = b - a, lo = a + len * part / split, hi = a + len * (part + 1) / split;
        a = lo;
        b = hi;
    }
    const uint32_t bmask = (1u << vbits) - 1u;
    constexpr uint32_t NONE = (uint32_t)(WORD)~(WORD)0;
    // (one workgroup per CU -- the histogram fills LDS -- so nothing else hides the load latency: the next batch's 8 loads per
    // lane are issued before this batch's adds)
    auto fetch = [&](int64_t base, uint32_t (&e)[8]) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t i = base + (int64_t)j * BIG_BLOCK + threadIdx.x;
            if (sizeof(WORD) == 2) {
                // (through the dword that holds it: two lanes share a load, and the compiler does not serialise dword loads the
                // way it does 2-byte ones -- it put s_waitcnt vmcnt(0) behind every global_load_ushort)
                const uint32_t pair = i < b ? reinterpret_cast<const uint32_t *>(words)[i >> 1] : 0xffffffffu;
                e[j] = (i & 1) ? pair >> 16 : pair & 0xffffu;
            } else {
                e[j] = i < b ? (uint32_t)words[i] : NONE;
            }
        }
    };
    uint32_t e[8], en[8];
    fetch(a, e);
    for (int64_t base = a; base < b; base += (int64_t)BIG_BLOCK * 8) {
        fetch(base + (int64_t)BIG_BLOCK * 8, en);
        // equal words in neighbouring lanes are added once: consecutive k-mers of a read share their row and, mostly, their bin,
        // and a lookup pass that works on super-k-mers leaves them next to each other -- as single adds they would queue up on
        // one LDS address
        const uint32_t lane = threadIdx.x & 63;
        if (COUNTED) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (e[j] != NONE)
                    atomicAdd(&hist[((e[j] >> vbits) & ((1u << GROUP_ROWS_LOG2) - 1u)) * stride + (e[j] & bmask)], (e[j] >> PG_SHUFFLE_COUNT_SHIFT) + 1u);
        } else
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t prev = __shfl_up(e[j], 1);
            const bool head = lane == 0 || e[j] != prev;
            const unsigned long long hm = __ballot(head);
            const unsigned long long above = lane == 63 ? 0ull : hm >> (lane + 1);
            const uint32_t run = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
            if (head && e[j] != NONE) atomicAdd(&hist[((e[j] >> vbits) & ((1u << GROUP_ROWS_LOG2) - 1u)) * stride + (e[j] & bmask)], run);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = en[j];
    }
    __syncthreads();
    int32_t *dst = abd_out + row0 * (int64_t)vsize;
    const uint32_t n_out = (uint32_t)rows_here * vsize;
    if (split > 1) {
        for (uint32_t i = threadIdx.x; i < n_out; i += BIG_BLOCK) {
            const uint32_t v = hist[(i / vsize) * stride + i % vsize];
            if (v) atomicAdd(&dst[i], (int32_t)v);
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < n_out; i += BIG_BLOCK) dst[i] = (int32_t)hist[(i / vsize) * stride + i % vsize];
}

// -------------------------------------------------------------------------------- K1 + K3 by lookups: per-run rows

// LDS: abd_copies x [vsize] abundance bins, then tnf_copies x [4^k_tnf] raw k_tnf-mer bins
// (one copy per wavefront while that fits comfortably, else one shared copy).
template <typename KT, int TK>
__global__ __launch_bounds__(BLOCK) void features_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                         int64_t n_words, const int32_t *__restrict__ seg_row,
                                                         const int64_t *__restrict__ seg_start, const int64_t *__restrict__ seg_end,
                                                         int k_tnf, const uint16_t *__restrict__ colmap, int tnf_cols, int tnf_copies, int abd_copies,
                                                         int32_t *__restrict__ tnf_out, int k, const uint32_t *__restrict__ dense, HashView t,
                                                         uint32_t window, int vsize, int32_t *__restrict__ abd_out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const bool do_tnf = tnf_out != nullptr;
    const bool do_abd = TK != TK_NONE && abd_out != nullptr;
    const int n_raw = do_tnf ? 1 << (2 * k_tnf) : 0;
    const int abd_bins = do_abd ? vsize : 0;
    uint32_t *abd_lds = lds;
    uint32_t *tnf_lds = lds + abd_copies * abd_bins;
    const int lds_words = abd_copies * abd_bins + tnf_copies * n_raw;
    for (int i = threadIdx.x; i < lds_words; i += BLOCK) lds[i] = 0;
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    uint32_t *my_abd = abd_lds + (abd_copies > 1 ? wave * abd_bins : 0);
    uint32_t *my_tnf = tnf_lds + (tnf_copies > 1 ? wave * n_raw : 0);

    const int64_t s0 = seg_start[blockIdx.x], s1 = seg_end[blockIdx.x];
    const int kk = do_abd ? k : k_tnf;                                       // what the roller rolls
    const int kroll = do_abd ? (k > k_tnf || !do_tnf ? k : k_tnf) : k_tnf;   // characters to pre-roll + 1
    const uint32_t tmask = do_tnf ? (uint32_t)n_raw - 1u : 0u;

    for (int64_t w = (s0 >> 5) + threadIdx.x; w <= ((s1 - 1) >> 5) && w < n_words; w += BLOCK) {
        const uint64_t cw = codes[w];
        const uint32_t vw = valid[w];
        const uint64_t pw = w > 0 ? codes[w - 1] : 0;
        const uint32_t pv = w > 0 ? valid[w - 1] : 0;
        // characters of this word that belong to the segment
        const int64_t base = w << 5;
        const int lo = s0 > base ? (int)(s0 - base) : 0;
        const int hi = s1 < base + 32 ? (int)(s1 - base) : 32;
        uint32_t in_seg = (hi >= 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
        const uint64_t m = ((uint64_t)vw << 32) | pv;
        const uint32_t ok_t = do_tnf ? (uint32_t)(runs_of(m, k_tnf) >> 32) & in_seg : 0u;
        const uint32_t ok_a = do_abd ? (uint32_t)(runs_of(m, k) >> 32) & in_seg : 0u;
        if ((ok_t | ok_a) == 0) continue;

        Roller<KT> r;
        r.init(kk);
        for (int i = 33 - kroll; i < 32; ++i) r.push((uint32_t)(pw >> (2 * i)) & 3u);
        // batches of 8 characters: roll, issue the table reads of the batch, then bin them
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            KT canon[8];
            uint64_t cur[8];
            uint64_t hh[8];
            uint64_t key8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = b * 8 + u;
                r.push((uint32_t)(cw >> (2 * j)) & 3u);
                if (do_tnf && ((ok_t >> j) & 1)) atomicAdd(&my_tnf[(uint32_t)r.fw & tmask], 1u);
                if (TK != TK_NONE) {
                    canon[u] = r.canon();
                    cur[u] = 0;
                    if ((ok_a >> j) & 1) {
                        if (TK == TK_DENSE) {
                            cur[u] = dense[(uint32_t)canon[u]];
                        } else {
                            key8[u] = TK == TK_HASH ? key42((uint64_t)canon[u]) : (uint64_t)canon[u];
                            hh[u] = TK == TK_WIDE ? t.home_wide(key8[u]) : (TK == TK_MINI || TK == TK_MINIW) ? t.home_mini(key8[u], k) : t.home_key(key8[u]);
                            // each table line is used once per launch: keep it out of the way of the stream (measured -2 %)
                            cur[u] = __builtin_nontemporal_load(&t.slots[hh[u]]);
                        }
                    }
                }
            }
            if (TK != TK_NONE) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int j = b * 8 + u;
                    if ((ok_a >> j) & 1) {
                        uint32_t cnt;
                        bool found = true;
                        if (TK == TK_DENSE) {
                            cnt = (uint32_t)cur[u];
                            found = cnt != 0;       // absent from the table <=> never counted
                        } else if (TK == TK_WIDE || TK == TK_MINIW) {
                            cnt = wide_probe(t, hh[u], cur[u], key8[u], &found);
                        } else {
                            cnt = hash_probe(t, hh[u], cur[u], key8[u], &found);
                        }
                        if (found) {
                            uint32_t bin = cnt / window;
                            if (bin < (uint32_t)vsize) atomicAdd(&my_abd[bin], 1u);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();

    const int64_t row = seg_row[blockIdx.x];
    if (do_abd) {
        for (int i = threadIdx.x; i < abd_bins; i += BLOCK) {
            uint32_t s = 0;
            for (int c = 0; c < abd_copies; ++c) s += abd_lds[c * abd_bins + i];
            if (s) atomicAdd(&abd_out[row * vsize + i], (int32_t)s);
        }
    }
    if (do_tnf) {
        for (int i = threadIdx.x; i < n_raw; i += BLOCK) {
            uint32_t s = 0;
            for (int c = 0; c < tnf_copies; ++c) s += tnf_lds[c * n_raw + i];
            if (s) atomicAdd(&tnf_out[row * tnf_cols + colmap[i]], (int32_t)s);
        }
    }
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

// one lookup in two halves, so that a lane issues the first probes of a batch before it resolves any (table_query_kernel)
struct DepthProbe {
    uint64_t key, hh, cur;
};
template <int TK>
__device__ __forceinline__ void depth_issue(DepthProbe &p, uint64_t canon, int k, const uint32_t *__restrict__ dense, const HashView &t)
{
    if (TK == TK_DENSE) {
        p.cur = dense[(uint32_t)canon];
        return;
    }
    p.key = TK == TK_HASH ? key42(canon) : canon;
    p.hh = TK == TK_WIDE ? t.home_wide(canon) : (TK == TK_MINI || TK == TK_MINIW) ? t.home_mini(canon, k) : t.home_key(p.key);
    p.cur = t.slots[p.hh];
}
template <int TK> __device__ __forceinline__ uint32_t depth_resolve(const DepthProbe &p, const HashView &t)
{
    bool found;
    if (TK == TK_DENSE) return (uint32_t)p.cur;
    if (TK == TK_WIDE || TK == TK_MINIW) return wide_probe(t, p.hh, p.cur, p.key, &found);
    return hash_probe(t, p.hh, p.cur, p.key, &found);
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
        DepthProbe p[DEPTH_BATCH];
        bool ask[DEPTH_BATCH];
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = g0 + u * stride, i = begin + g;
            uint64_t canon = 0;
            p[u].key = p[u].hh = p[u].cur = 0;
            ask[u] = g < n && i + k <= n_chars && kmer_at(codes, valid, i, k, kmask, &canon);
            if (ask[u]) depth_issue<TK>(p[u], canon, k, dense, t);
        }
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = g0 + u * stride;
            if (g < n) out[g] = ask[u] ? depth_resolve<TK>(p[u], t) : PG_PROFILE_NONE;
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
        DepthProbe p[DEPTH_BATCH];
        bool have[DEPTH_BATCH];
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = lane + 64 * u;
            uint64_t canon = 0;
            p[u].key = p[u].hh = p[u].cur = 0;
            have[u] = g < n_pos && kmer_at(codes, valid, a + g, k, kmask, &canon);
            if (have[u]) depth_issue<TK>(p[u], canon, k, dense, t);
        }
        uint32_t n = 0, present = 0, vmax = 0;
        unsigned long long sum = 0;
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            uint32_t c = have[u] ? depth_resolve<TK>(p[u], t) : 0u;
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
        DepthProbe p[DEPTH_BATCH];
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
            if (ask[u]) depth_issue<TK>(p[u], canon, k, dense, t);
        }
#pragma unroll
        for (int u = 0; u < DEPTH_BATCH; ++u) {
            const int64_t g = t0 + u * BLOCK + threadIdx.x;
            if (g < total) counts[g] = ask[u] ? depth_resolve<TK>(p[u], t) : PG_PROFILE_NONE;
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

// -------------------------------------------------------------------------------- launch helpers
int check_table(const pg_table *t)
{
    if (!t || !t->data) return pg_fail(PG_EINVAL, "table descriptor is null");
    if (t->kind == PG_TABLE_DENSE) {
        if (t->k < 1 || t->k > PG_DENSE_MAX_K) return pg_fail(PG_EINVAL, "dense table needs 1 <= k <= %d (got %d)", PG_DENSE_MAX_K, t->k);
    } else if (t->kind == PG_TABLE_HASH) {
        if (t->k < 1 || t->k > PG_HASH_MAX_K) return pg_fail(PG_EINVAL, "hash table needs 1 <= k <= %d (got %d)", PG_HASH_MAX_K, t->k);
        if (t->log2_slots < 10 || t->log2_slots > 40) return pg_fail(PG_EINVAL, "log2_slots %d out of range [10,40]", t->log2_slots);
        if (t->log2_bucket_slots != 0 && (t->log2_bucket_slots < 4 || t->log2_bucket_slots > t->log2_slots))
            return pg_fail(PG_EINVAL, "log2_bucket_slots %d out of range [4,%d]", t->log2_bucket_slots, t->log2_slots);
    } else if (t->kind == PG_TABLE_MINI) {
        if (t->k < PG_MINI_MIN_K || t->k > PG_HASH_MAX_K) return pg_fail(PG_EINVAL, "mini table needs %d <= k <= %d (got %d)", PG_MINI_MIN_K, PG_HASH_MAX_K, t->k);
        if (t->log2_bucket_slots < 4 || t->log2_bucket_slots > PG_BUCKET_MAX_LOG2_SLOTS || t->log2_slots < t->log2_bucket_slots ||
            t->log2_slots - t->log2_bucket_slots > PG_MINI_MAX_LOG2_BUCKETS)
            return pg_fail(PG_EINVAL, "mini table geometry 2^%d slots in buckets of 2^%d", t->log2_slots, t->log2_bucket_slots);
    } else if (t->kind == PG_TABLE_MINI_WIDE) {
        if (t->k <= PG_HASH_MAX_K || t->k > PG_WIDE_MAX_K) return pg_fail(PG_EINVAL, "wide mini table needs %d < k <= %d (got %d)", PG_HASH_MAX_K, PG_WIDE_MAX_K, t->k);
        if (t->log2_bucket_slots < 4 || t->log2_bucket_slots > PG_MINI_WIDE_MAX_LOG2_BUCKET_SLOTS || t->log2_slots < t->log2_bucket_slots ||
            t->log2_slots - t->log2_bucket_slots > PG_MINI_MAX_LOG2_BUCKETS)
            return pg_fail(PG_EINVAL, "wide mini table geometry 2^%d slots in buckets of 2^%d", t->log2_slots, t->log2_bucket_slots);
    } else if (t->kind == PG_TABLE_WIDE) {
        if (t->k < 1 || t->k > PG_WIDE_MAX_K) return pg_fail(PG_EINVAL, "wide table needs 1 <= k <= %d (got %d)", PG_WIDE_MAX_K, t->k);
        if (t->log2_slots < 10 || t->log2_slots > 40) return pg_fail(PG_EINVAL, "log2_slots %d out of range [10,40]", t->log2_slots);
        if (t->log2_bucket_slots != 0) return pg_fail(PG_EINVAL, "wide tables are not bucketed");
    } else {
        return pg_fail(PG_EINVAL, "unknown table kind %d", t->kind);
    }
    return PG_OK;
}

HashView view_of(const pg_table *t)
{
    HashView v;
    v.slots = (uint64_t *)t->data;
    v.log2_slots = t->log2_slots;
    v.log2_bucket = t->log2_bucket_slots ? t->log2_bucket_slots : t->log2_slots;
    return v;
}

// workspace carving of the bucketed counter
struct BucketPlan {
    int bits, bits1, bits2;           // bucket id bits, split over the two scatter passes
    int64_t cap, n_tiles, n_chunks;   // record capacity of each record buffer; stream tiles and chunks of the range
    size_t hist_off, off_off, cur1_off, cur2_off, tile_off, chunk_off, bufa_off, bufb_off, total;
    size_t final_off() const { return bits2 ? bufb_off : bufa_off; }
};

int plan_buckets(const pg_table *t, int64_t n_words, BucketPlan *p)
{
    if (t->kind != PG_TABLE_HASH || t->log2_bucket_slots == 0)
        return pg_fail(PG_EINVAL, "bucketed counting needs a hash table with log2_bucket_slots set");
    if (t->log2_bucket_slots > PG_BUCKET_MAX_LOG2_SLOTS)
        return pg_fail(PG_EINVAL, "log2_bucket_slots %d exceeds the LDS-resident maximum %d", t->log2_bucket_slots, PG_BUCKET_MAX_LOG2_SLOTS);
    p->bits = t->log2_slots - t->log2_bucket_slots;
    if (p->bits < 1 || p->bits > PG_BUCKET_MAX_LOG2_BUCKETS)
        return pg_fail(PG_EINVAL, "bucketed counting needs 1 <= log2_slots - log2_bucket_slots <= %d (got %d)", PG_BUCKET_MAX_LOG2_BUCKETS, p->bits);
    p->bits1 = p->bits < 8 ? p->bits : 8;
    p->bits2 = p->bits - p->bits1;
    if (p->bits2 > MAX_FAN_BITS) return pg_fail(PG_EINVAL, "too many buckets for two scatter passes");
    p->cap = n_words * 32;
    p->n_tiles = (n_words + TILE_WORDS - 1) / TILE_WORDS;
    p->n_chunks = (n_words + CHUNK_WORDS - 1) / CHUNK_WORDS;
    const size_t nb = (size_t)1 << p->bits;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    p->hist_off = take(nb * 8);
    p->off_off = take((nb + 1) * 8);
    p->cur1_off = take(((size_t)1 << p->bits1) * 8);
    p->cur2_off = take(nb * 8);
    p->tile_off = take((size_t)(p->n_tiles + 1) * 4);
    p->chunk_off = take(((size_t)p->n_chunks << p->bits1) * 8);
    p->bufa_off = take((size_t)p->cap * 8);
    p->bufb_off = p->bits2 ? take((size_t)p->cap * 8) : p->bufa_off;
    p->total = o;
    return PG_OK;
}

int check_rows(const pg_rows *rows, const char *who)
{
    if (!rows) return PG_OK;
    if (rows->n_rows < 0 || rows->n_rows >= (int64_t)ROW_NONE)
        return pg_fail(PG_EINVAL, "%s: %lld rows (at most %u per launch)", who, (long long)rows->n_rows, ROW_NONE - 1);
    if (rows->n_rows > 0 && (!rows->row_start || !rows->row_end)) return pg_fail(PG_EINVAL, "%s: null row arrays", who);
    return PG_OK;
}

// carving of the shuffle workspace
struct ShufflePlan {
    int vbits, gbits, gb1, gb2;
    int64_t n_groups, n_groups_padded;
    size_t emit_off, caps_off, goff_off, gcur1_off, gcur2_off, dhist_off, words_e_off, words_a_off, words_b_off, total;
};

// no_input (callers that keep their provisional data elsewhere -- the merged lookups of mini.hip): when one scatter pass suffices the
// first word buffer is not needed at all (12 GB per 10 M read pairs that were allocated and never touched)
int plan_shuffle(int64_t cap, int64_t n_rows, int vsize, int64_t n_buckets, ShufflePlan *p, int one_pass_bits = WIDE_FAN_BITS, int no_input = 0)
{
    if (vsize < 1 || vsize > PG_SHUFFLE_MAX_VSIZE)
        return pg_fail(PG_EINVAL, "the shuffle path needs 1 <= vector size <= %d (got %d)", PG_SHUFFLE_MAX_VSIZE, vsize);
    p->vbits = 1;
    while ((1 << p->vbits) < vsize) ++p->vbits;
    p->n_groups = (n_rows + (1 << GROUP_ROWS_LOG2) - 1) >> GROUP_ROWS_LOG2;
    if (p->n_groups < 1) p->n_groups = 1;
    p->gbits = 0;
    while (((int64_t)1 << p->gbits) < p->n_groups) ++p->gbits;
    p->gb1 = p->gbits < 8 ? p->gbits : 8;
    // one pass up to 2^one_pass_bits row groups: 2^10 (65536 rows) for the scatter kernels of this file; a lookup pass that
    // scatters by itself may manage more (mini.hip: 2^11)
    if (p->gbits <= one_pass_bits && !getenv("PG_S2_TWO_PASS")) p->gb1 = p->gbits;
    p->gb2 = p->gbits - p->gb1;
    if (p->gb2 > MAX_FAN_BITS) return pg_fail(PG_EINVAL, "too many rows for two scatter passes");
    p->n_groups_padded = (int64_t)1 << p->gbits;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    p->emit_off = take(((size_t)1 << PG_BUCKET_MAX_LOG2_BUCKETS) * 8);
    p->caps_off = take((size_t)p->n_groups_padded * 8);
    p->goff_off = take((size_t)(p->n_groups_padded + 1) * 8);
    p->gcur1_off = take(((size_t)1 << p->gb1) * 8);
    p->gcur2_off = take((size_t)p->n_groups_padded * 8);
    p->dhist_off = o;
    (void)n_buckets;
    p->words_e_off = take(no_input && p->gb2 == 0 ? 0 : (size_t)cap * 4);   // emitted by the lookup pass, bucket order
    p->words_a_off = take((size_t)cap * 4);                              // after the first row pass
    p->words_b_off = p->gb2 ? p->words_e_off : p->words_a_off;           // the second row pass reuses the first buffer
    p->total = o;
    return PG_OK;
}

}  // namespace

extern "C" int pg_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return pg_fail(PG_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

extern "C" int pg_kmer_count(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                             const pg_table *t, uint32_t *status, void *stream)
{
    if (!codes || !valid) return pg_fail(PG_EINVAL, "pg_kmer_count: null stream arrays");
    if (word_begin < 0 || word_end < word_begin) return pg_fail(PG_EINVAL, "pg_kmer_count: bad word range [%lld,%lld)", (long long)word_begin, (long long)word_end);
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind == PG_TABLE_MINI || t->kind == PG_TABLE_MINI_WIDE) return pg_fail(PG_EINVAL, "pg_kmer_count: mini tables are built by pg_mini_plan + pg_mini_count");
    if (t->kind != PG_TABLE_DENSE && !status) return pg_fail(PG_EINVAL, "pg_kmer_count: hash tables need a status word");
    if (word_end == word_begin) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    int grid = grid_for(word_end - word_begin);
    if (t->kind == PG_TABLE_DENSE) {
        HashView none{nullptr, 0, 0};
        hipLaunchKernelGGL((kmer_count_kernel<uint32_t, TK_DENSE>), dim3(grid), dim3(BLOCK), 0, s, codes, valid, word_begin, word_end,
                           t->k, (uint32_t *)t->data, none, status);
    } else if (t->kind == PG_TABLE_WIDE) {
        hipLaunchKernelGGL((kmer_count_kernel<uint64_t, TK_WIDE>), dim3(grid), dim3(BLOCK), 0, s, codes, valid, word_begin, word_end,
                           t->k, (uint32_t *)nullptr, view_of(t), status);
    } else {
        hipLaunchKernelGGL((kmer_count_kernel<uint64_t, TK_HASH>), dim3(grid), dim3(BLOCK), 0, s, codes, valid, word_begin, word_end,
                           t->k, (uint32_t *)nullptr, view_of(t), status);
    }
    return check_launch("pg_kmer_count");
}

extern "C" int pg_kmer_distinct_sketch(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, int k,
                                       uint32_t *registers, void *stream)
{
    if (!codes || !valid || !registers) return pg_fail(PG_EINVAL, "pg_kmer_distinct_sketch: null argument");
    if (k < 1 || k > PG_WIDE_MAX_K) return pg_fail(PG_EINVAL, "pg_kmer_distinct_sketch: k %d out of range", k);
    if (word_begin < 0 || word_end < word_begin) return pg_fail(PG_EINVAL, "pg_kmer_distinct_sketch: bad word range");
    if (word_end == word_begin) return PG_OK;
    int grid = (int)((word_end - word_begin + BIG_BLOCK - 1) / BIG_BLOCK);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(distinct_sketch_kernel, dim3(grid), dim3(BIG_BLOCK), 0, (hipStream_t)stream, codes, valid, word_begin, word_end, k, registers);
    return check_launch("pg_kmer_distinct_sketch");
}

extern "C" int64_t pg_kmer_count_workspace_bytes(int64_t n_words, const pg_table *t)
{
    if (n_words < 0) return pg_fail(PG_EINVAL, "negative word count");
    int rc = check_table(t);
    if (rc) return rc;
    BucketPlan p;
    rc = plan_buckets(t, n_words, &p);
    if (rc) return rc;
    return (int64_t)p.total;
}

namespace {
struct EmitArgs { int window, vsize; void *shuffle_ws; int64_t shuffle_ws_bytes; };     // fused count + lookup (one GPU)
int count_bucketed_impl(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                        const pg_table *t, int accumulate, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                        uint32_t *status, void *stream, int deferred_group, int64_t *fill, const EmitArgs *emit = nullptr);
}

extern "C" int pg_kmer_count_bucketed(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                                      const pg_table *t, int accumulate, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                                      uint32_t *status, void *stream)
{
    return count_bucketed_impl(codes, valid, word_begin, word_end, t, accumulate, rows, workspace, workspace_bytes, status, stream, -1, nullptr);
}

extern "C" int pg_kmer_count_deferred(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                                      const pg_table *t, int group_log2, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                                      int64_t *fill, uint32_t *status, void *stream)
{
    if (group_log2 < 0 || group_log2 > PG_DEFERRED_MAX_GROUP_LOG2) return pg_fail(PG_EINVAL, "pg_kmer_count_deferred: group_log2 %d not in [0,%d]", group_log2, PG_DEFERRED_MAX_GROUP_LOG2);
    if (!fill) return pg_fail(PG_EINVAL, "pg_kmer_count_deferred: null fill array");
    return count_bucketed_impl(codes, valid, word_begin, word_end, t, 0, rows, workspace, workspace_bytes, status, stream, group_log2, fill);
}

extern "C" int pg_deferred_gather(const pg_table *t, const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                                  const int64_t *fill, const int64_t *seg, uint64_t *out, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (!count_workspace || !fill || !seg || !out) return pg_fail(PG_EINVAL, "pg_deferred_gather: null argument");
    BucketPlan p;
    if ((rc = plan_buckets(t, n_words_counted, &p))) return rc;
    if (!p.bits2) return pg_fail(PG_EINVAL, "pg_deferred_gather: the deferred form needs more than 256 buckets");
    if ((int64_t)p.total > count_workspace_bytes) return pg_fail(PG_EINVAL, "pg_deferred_gather: count workspace does not match n_words_counted");
    const char *ws = (const char *)count_workspace;
    const int64_t nb = (int64_t)1 << p.bits;
    hipLaunchKernelGGL(deferred_gather_kernel, dim3((unsigned)((nb + WAVES - 1) / WAVES)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)(ws + p.bufa_off), (const unsigned long long *)(ws + p.off_off), (const long long *)fill,
                       (const long long *)seg, nb, out);
    return check_launch("pg_deferred_gather");
}

extern "C" int pg_deferred_gather_planes(const pg_table *t, const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                                         const int64_t *fill, const int64_t *tag_elem, const int64_t *cnt_elem, void *out,
                                         uint64_t *overflow, uint64_t *overflow_count, int64_t overflow_cap, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (!count_workspace || !fill || !tag_elem || !cnt_elem || !out || !overflow || !overflow_count || !status)
        return pg_fail(PG_EINVAL, "pg_deferred_gather_planes: null argument");
    BucketPlan p;
    if ((rc = plan_buckets(t, n_words_counted, &p))) return rc;
    if (!p.bits2) return pg_fail(PG_EINVAL, "pg_deferred_gather_planes: the deferred form needs more than 256 buckets");
    if (KEY_BITS - p.bits > 31) return pg_fail(PG_EINVAL, "pg_deferred_gather_planes: needs at least 2^11 buckets (tags of at most 31 bits)");
    if ((int64_t)p.total > count_workspace_bytes) return pg_fail(PG_EINVAL, "pg_deferred_gather_planes: count workspace does not match n_words_counted");
    const char *ws = (const char *)count_workspace;
    const int64_t nb = (int64_t)1 << p.bits;
    hipLaunchKernelGGL(deferred_gather_planes_kernel, dim3((unsigned)((nb + WAVES - 1) / WAVES)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)(ws + p.bufa_off), (const unsigned long long *)(ws + p.off_off), (const long long *)fill,
                       (const long long *)tag_elem, (const long long *)cnt_elem, nb, (uint32_t)((1u << (KEY_BITS - p.bits)) - 1u),
                       (uint32_t *)out, (uint16_t *)out, overflow, (unsigned long long *)overflow_count, (unsigned long long)overflow_cap, status);
    return check_launch("pg_deferred_gather_planes");
}

extern "C" int pg_kmer_rebuild_planes_range(const void *buf, int64_t part_stride_bytes, int64_t cap, const int64_t *seg, int n_parts,
                                            const pg_table *t, int64_t bucket_begin, int64_t bucket_end, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind != PG_TABLE_HASH || t->log2_bucket_slots == 0 || t->log2_bucket_slots > PG_BUCKET_MAX_LOG2_SLOTS)
        return pg_fail(PG_EINVAL, "pg_kmer_rebuild_planes_range: needs a bucketed hash table with LDS-sized buckets");
    const int bits = t->log2_slots - t->log2_bucket_slots;
    if (KEY_BITS - bits > 31) return pg_fail(PG_EINVAL, "pg_kmer_rebuild_planes_range: needs at least 2^11 buckets (tags of at most 31 bits)");
    if (n_parts < 1 || !buf || !seg || !status || cap < 0 || part_stride_bytes < 6 * cap) return pg_fail(PG_EINVAL, "pg_kmer_rebuild_planes_range: bad arguments");
    if (bucket_begin < 0 || bucket_end < bucket_begin || bucket_end > ((int64_t)1 << bits))
        return pg_fail(PG_EINVAL, "pg_kmer_rebuild_planes_range: bucket range [%lld,%lld) outside the table", (long long)bucket_begin, (long long)bucket_end);
    if (bucket_end == bucket_begin) return PG_OK;
    const size_t lds = (size_t)8 << t->log2_bucket_slots;
    if ((rc = raise_lds_limit((const void *)bucket_merge_planes_kernel, lds, "pg_kmer_rebuild_planes_range"))) return rc;
    hipLaunchKernelGGL(bucket_merge_planes_kernel, dim3((unsigned)(bucket_end - bucket_begin)), dim3(BIG_BLOCK), lds, (hipStream_t)stream,
                       (const uint8_t *)buf, part_stride_bytes, cap, (const long long *)seg, n_parts, view_of(t), status, bucket_begin,
                       bucket_end - bucket_begin);
    return check_launch("pg_kmer_rebuild_planes_range");
}

extern "C" int pg_kmer_count_bucketed_emit(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                                           const pg_table *t, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                                           int window, int vsize, void *shuffle_workspace, int64_t shuffle_workspace_bytes,
                                           uint32_t *status, void *stream)
{
    if (!rows || rows->n_rows < 1) return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed_emit: needs rows");
    if (!shuffle_workspace) return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed_emit: null shuffle workspace");
    if (window < 1 || (int64_t)window * vsize > (int64_t)PG_HASH_COUNT_SAT)
        return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed_emit: window %d x vector size %d outside the exact range of the hash table", window, vsize);
    const EmitArgs e{window, vsize, shuffle_workspace, shuffle_workspace_bytes};
    return count_bucketed_impl(codes, valid, word_begin, word_end, t, 0, rows, workspace, workspace_bytes, status, stream, -1, nullptr, &e);
}

namespace {
int count_bucketed_impl(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                        const pg_table *t, int accumulate, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                        uint32_t *status, void *stream, int deferred_group, int64_t *fill, const EmitArgs *emit)
{
    if (!codes || !valid || !workspace || !status) return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed: null argument");
    if (word_begin < 0 || word_end < word_begin) return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed: bad word range");
    int rc = check_table(t);
    if (rc) return rc;
    if ((rc = check_rows(rows, "pg_kmer_count_bucketed"))) return rc;
    BucketPlan p;
    rc = plan_buckets(t, word_end - word_begin, &p);
    if (rc) return rc;
    if ((int64_t)p.total > workspace_bytes)
        return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)p.total);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (deferred_group >= 0) {
        if (!p.bits2) return pg_fail(PG_EINVAL, "pg_kmer_count_deferred: the deferred form needs more than 256 buckets");
        if (deferred_group > p.bits2) return pg_fail(PG_EINVAL, "pg_kmer_count_deferred: group_log2 %d exceeds the second-pass bits %d", deferred_group, p.bits2);
        if (word_end == word_begin) {
            if (hipMemsetAsync(fill, 0, sizeof(int64_t) << p.bits, s) != hipSuccess) return pg_fail(PG_EHIP, "pg_kmer_count_deferred: memset failed");
            return PG_OK;
        }
    }
    if (word_end == word_begin) return PG_OK;
    char *ws = (char *)workspace;
    auto *hist = (unsigned long long *)(ws + p.hist_off);
    auto *off = (unsigned long long *)(ws + p.off_off);
    auto *cur2 = (unsigned long long *)(ws + p.cur2_off);
    auto *tile_row = (int32_t *)(ws + p.tile_off);
    auto *chunk_tab = (unsigned long long *)(ws + p.chunk_off);
    auto *bufa = (uint64_t *)(ws + p.bufa_off);
    auto *bufb = (uint64_t *)(ws + p.bufb_off);
    const int nb = 1 << p.bits;
    // counters are contiguous at the front of the workspace: one clear
    if (hipMemsetAsync(ws, 0, p.tile_off, s) != hipSuccess) return pg_fail(PG_EHIP, "pg_kmer_count_bucketed: memset failed");
    const size_t slice_lds = (size_t)8 << t->log2_bucket_slots;
    const int hist_bins = nb < (1 << 15) ? nb : (1 << 15);
    const size_t hist_lds = (size_t)hist_bins * 4 + 1024;
    if ((rc = raise_lds_limit((const void *)bucket_hist_kernel, hist_lds, "pg_kmer_count_bucketed"))) return rc;
    if ((rc = raise_lds_limit((const void *)bucket_count_kernel, slice_lds, "pg_kmer_count_bucketed"))) return rc;

    const bool with_rows = rows && rows->n_rows > 0;
    if (with_rows)
        hipLaunchKernelGGL(tile_rows_kernel, dim3((unsigned)((p.n_tiles + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, rows->row_end, rows->n_rows,
                           word_begin, p.n_tiles, tile_row);
    // golden-ratio stride, made coprime to the chunk count: a bijection on chunk indices
    int64_t chunk_stride = (int64_t)((double)p.n_chunks * 0.6180339887) | 1;
    {
        auto gcd = [](int64_t a, int64_t b) { while (b) { int64_t t = a % b; a = b; b = t; } return a; };
        while (gcd(chunk_stride, p.n_chunks) != 1) chunk_stride += 2;
    }
    // A0 histogram of final bucket ids + per-chunk first-digit counts, then offsets of buckets and of chunks
    {
        const int grid = (int)(p.n_chunks < 512 ? p.n_chunks : 512);
        for (int base = 0; base < nb; base += hist_bins)
            hipLaunchKernelGGL(bucket_hist_kernel, dim3(grid), dim3(BIG_BLOCK), hist_lds, s, codes, valid, word_begin, word_end,
                               t->k, p.bits, (uint32_t)base, hist_bins, hist, p.bits1, base == 0 ? chunk_tab : (unsigned long long *)nullptr, p.n_chunks,
                               chunk_stride);
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)hist, (int64_t)nb, off);
        hipLaunchKernelGGL(digit_scan_kernel, dim3(1u << p.bits1), dim3(BIG_BLOCK), 0, s, chunk_tab, p.n_chunks, (const unsigned long long *)off,
                           p.bits2, (unsigned long long *)nullptr);
    }
    // A1: stream -> 2^bits1 regions (region d1 = final buckets [d1 << bits2, (d1+1) << bits2)); one workgroup per chunk
    hipLaunchKernelGGL(scatter_stream_kernel, dim3((unsigned)p.n_chunks), dim3(BLOCK), 0, s, codes, valid, word_begin, word_end, t->k, p.bits1,
                       with_rows ? rows->row_start : (const int64_t *)nullptr, with_rows ? rows->row_end : (const int64_t *)nullptr,
                       with_rows ? rows->n_rows : (int64_t)0, with_rows ? rows->strict_valid : (const uint32_t *)nullptr,
                       (const int32_t *)tile_row, bufa, (const unsigned long long *)chunk_tab, p.n_chunks,
                       chunk_stride);
    // A2: every region -> its 2^bits2 final buckets
    if (p.bits2) {
        const int tiles_x = 96;
        hipLaunchKernelGGL((scatter_records_kernel<uint64_t, DIG_HASH, RPL64, MAX_FAN_BITS>), dim3((unsigned)(tiles_x << p.bits1)), dim3(BLOCK), 0, s,
                           (const uint64_t *)bufa, (const unsigned long long *)off, (const unsigned long long *)(off + ((size_t)1 << p.bits2)),
                           p.bits2, (const unsigned long long *)nullptr, tiles_x, bufb, (const unsigned long long *)off, cur2, 0, 0,
                           p.bits2, KEY_BITS - p.bits);
    }
    if (deferred_group >= 0) {
        // B, deferred: groups of final buckets counted in LDS, occupied entries + fills only (bufa is free after A2)
        const bool split32 = KEY_BITS - (p.bits - deferred_group) <= 31 && !getenv("PG_B64");
        const void *fn = split32 ? (const void *)bucket_count_compact32_kernel : (const void *)bucket_count_compact_kernel;
        if ((rc = raise_lds_limit(fn, slice_lds, "pg_kmer_count_deferred"))) return rc;
        hipLaunchKernelGGL(split32 ? bucket_count_compact32_kernel : bucket_count_compact_kernel, dim3((unsigned)(nb >> deferred_group)),
                           dim3(BIG_BLOCK), slice_lds, s, (const uint64_t *)bufb,
                           (const unsigned long long *)off, view_of(t), deferred_group, bufa, (long long *)fill, status);
        return check_launch("pg_kmer_count_deferred");
    }
    if (emit) {
        // B + S1 fused: counts, slice image and the (row, bin) words of the abundance rows in one pass over the buckets
        if (KEY_BITS - p.bits > 31) return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed_emit: needs at least 2^11 buckets");
        ShufflePlan sp;
        if ((rc = plan_shuffle(p.cap, rows->n_rows, emit->vsize, (int64_t)nb, &sp))) return rc;
        if ((int64_t)sp.total > emit->shuffle_ws_bytes || (reinterpret_cast<uintptr_t>(emit->shuffle_ws) & 255) != 0)
            return pg_fail(PG_EINVAL, "pg_kmer_count_bucketed_emit: shuffle workspace of %lld bytes (256-byte aligned), %lld needed",
                           (long long)emit->shuffle_ws_bytes, (long long)sp.total);
        char *sws = (char *)emit->shuffle_ws;
        if ((rc = raise_lds_limit((const void *)bucket_count_emit32_kernel, slice_lds, "pg_kmer_count_bucketed_emit"))) return rc;
        hipLaunchKernelGGL(bucket_count_emit32_kernel, dim3(nb), dim3(BIG_BLOCK), slice_lds, s, (const uint64_t *)(p.bits2 ? bufb : bufa),
                           (const unsigned long long *)off, view_of(t), (uint32_t)emit->window, (uint32_t)emit->vsize, sp.vbits,
                           (uint32_t *)(sws + sp.words_e_off), (unsigned long long *)(sws + sp.emit_off), status);
        return check_launch("pg_kmer_count_bucketed_emit");
    }
    // B: count every bucket inside LDS and write its slice of the table
    if (KEY_BITS - p.bits <= 31 && !getenv("PG_B64")) {
        if ((rc = raise_lds_limit((const void *)bucket_count32_kernel, slice_lds, "pg_kmer_count_bucketed"))) return rc;
        hipLaunchKernelGGL(bucket_count32_kernel, dim3(nb), dim3(BIG_BLOCK), slice_lds, s, (const uint64_t *)(p.bits2 ? bufb : bufa),
                           (const unsigned long long *)off, view_of(t), accumulate ? 1 : 0, status);
    } else
    hipLaunchKernelGGL(bucket_count_kernel, dim3(nb), dim3(BIG_BLOCK), slice_lds, s, (const uint64_t *)(p.bits2 ? bufb : bufa),
                       (const unsigned long long *)off, view_of(t), accumulate ? 1 : 0, status);
    return check_launch("pg_kmer_count_bucketed");
}
}  // namespace

extern "C" int pg_kmer_merge(const uint64_t *pairs, int64_t n, const pg_table *t, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind != PG_TABLE_HASH && t->kind != PG_TABLE_MINI)
        return pg_fail(PG_EINVAL, "pg_kmer_merge: hash and mini tables only (dense tables are summed with an all-reduce)");
    if (n < 0 || (n > 0 && !pairs) || !status) return pg_fail(PG_EINVAL, "pg_kmer_merge: bad arguments");
    if (n == 0) return PG_OK;
    hipLaunchKernelGGL(kmer_merge_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, pairs, n, view_of(t), status,
                       t->kind == PG_TABLE_MINI ? t->k : 0);
    return check_launch("pg_kmer_merge");
}

extern "C" int pg_kmer_merge_wide(const uint64_t *codes, const uint32_t *counts, int64_t n, const pg_table *t, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind != PG_TABLE_WIDE && t->kind != PG_TABLE_MINI_WIDE) return pg_fail(PG_EINVAL, "pg_kmer_merge_wide: wide and wide mini tables only");
    if (n < 0 || (n > 0 && (!codes || !counts)) || !status) return pg_fail(PG_EINVAL, "pg_kmer_merge_wide: bad arguments");
    if (n == 0) return PG_OK;
    hipLaunchKernelGGL(wide_merge_kernel, dim3(grid_for(n)), dim3(BLOCK), 0, (hipStream_t)stream, codes, counts, n, view_of(t), status,
                       t->kind == PG_TABLE_MINI_WIDE ? t->k : 0);
    return check_launch("pg_kmer_merge_wide");
}

extern "C" int pg_kmer_merge_bucketed(const uint64_t *pairs, const int64_t *seg, int n_parts, const pg_table *t, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind != PG_TABLE_HASH || t->log2_bucket_slots == 0 || t->log2_bucket_slots > PG_BUCKET_MAX_LOG2_SLOTS)
        return pg_fail(PG_EINVAL, "pg_kmer_merge_bucketed: needs a bucketed hash table with LDS-sized buckets");
    if (n_parts < 0 || (n_parts > 0 && (!pairs || !seg)) || !status) return pg_fail(PG_EINVAL, "pg_kmer_merge_bucketed: bad arguments");
    if (n_parts == 0) return PG_OK;
    const int bits = t->log2_slots - t->log2_bucket_slots;
    if (bits < 0 || bits > 30) return pg_fail(PG_EINVAL, "pg_kmer_merge_bucketed: bad bucket geometry");
    const size_t lds = (size_t)8 << t->log2_bucket_slots;
    const bool split32 = KEY_BITS - bits <= 31 && !getenv("PG_B64");
    if ((rc = raise_lds_limit(split32 ? (const void *)bucket_merge32_kernel : (const void *)bucket_merge_kernel, lds, "pg_kmer_merge_bucketed"))) return rc;
    hipLaunchKernelGGL(split32 ? bucket_merge32_kernel : bucket_merge_kernel, dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, pairs, (const long long *)seg,
                       n_parts, view_of(t), status, 0, (int64_t)0, (int64_t)1 << bits);
    return check_launch("pg_kmer_merge_bucketed");
}

extern "C" int pg_kmer_rebuild_bucketed_range(const uint64_t *pairs, const int64_t *seg, int n_parts, const pg_table *t,
                                              int64_t bucket_begin, int64_t bucket_end, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind != PG_TABLE_HASH || t->log2_bucket_slots == 0 || t->log2_bucket_slots > PG_BUCKET_MAX_LOG2_SLOTS)
        return pg_fail(PG_EINVAL, "pg_kmer_rebuild_bucketed: needs a bucketed hash table with LDS-sized buckets");
    if (n_parts < 1 || !pairs || !seg || !status) return pg_fail(PG_EINVAL, "pg_kmer_rebuild_bucketed: bad arguments");
    const int bits = t->log2_slots - t->log2_bucket_slots;
    if (bits < 0 || bits > 30) return pg_fail(PG_EINVAL, "pg_kmer_rebuild_bucketed: bad bucket geometry");
    if (bucket_begin < 0 || bucket_end < bucket_begin || bucket_end > ((int64_t)1 << bits))
        return pg_fail(PG_EINVAL, "pg_kmer_rebuild_bucketed: bucket range [%lld,%lld) outside the table", (long long)bucket_begin, (long long)bucket_end);
    if (bucket_end == bucket_begin) return PG_OK;
    const size_t lds = (size_t)8 << t->log2_bucket_slots;
    const bool split32 = KEY_BITS - bits <= 31 && !getenv("PG_B64");
    if ((rc = raise_lds_limit(split32 ? (const void *)bucket_merge32_kernel : (const void *)bucket_merge_kernel, lds, "pg_kmer_rebuild_bucketed"))) return rc;
    hipLaunchKernelGGL(split32 ? bucket_merge32_kernel : bucket_merge_kernel, dim3((unsigned)(bucket_end - bucket_begin)), dim3(BIG_BLOCK), lds,
                       (hipStream_t)stream, pairs,
                       (const long long *)seg, n_parts, view_of(t), status, 1, bucket_begin, bucket_end - bucket_begin);
    return check_launch("pg_kmer_rebuild_bucketed");
}

extern "C" int pg_kmer_rebuild_bucketed(const uint64_t *pairs, const int64_t *seg, int n_parts, const pg_table *t, uint32_t *status, void *stream)
{
    int rc = check_table(t);
    if (rc) return rc;
    return pg_kmer_rebuild_bucketed_range(pairs, seg, n_parts, t, 0, (int64_t)1 << (t->log2_slots - t->log2_bucket_slots), status, stream);
}

static int check_bucketed(const pg_table *t, const char *who)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (t->kind != PG_TABLE_HASH || t->log2_bucket_slots < 1) return pg_fail(PG_EINVAL, "%s: needs a bucketed hash table", who);
    if (t->log2_slots - t->log2_bucket_slots > 30) return pg_fail(PG_EINVAL, "%s: too many buckets for one launch", who);
    return PG_OK;
}

extern "C" int pg_table_bucket_fill(const pg_table *t, int64_t *fill, void *stream)
{
    int rc = check_bucketed(t, "pg_table_bucket_fill");
    if (rc) return rc;
    if (!fill) return pg_fail(PG_EINVAL, "pg_table_bucket_fill: null output");
    hipLaunchKernelGGL(bucket_fill_kernel, dim3(1u << (t->log2_slots - t->log2_bucket_slots)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)t->data, t->log2_bucket_slots, (long long *)fill);
    return check_launch("pg_table_bucket_fill");
}

extern "C" int pg_table_bucket_fill_range(const pg_table *t, int64_t bucket_begin, int64_t bucket_end, int64_t *fill, void *stream)
{
    int rc = check_bucketed(t, "pg_table_bucket_fill_range");
    if (rc) return rc;
    const int64_t nb = (int64_t)1 << (t->log2_slots - t->log2_bucket_slots);
    if (!fill || bucket_begin < 0 || bucket_end < bucket_begin || bucket_end > nb) return pg_fail(PG_EINVAL, "pg_table_bucket_fill_range: bad arguments");
    if (bucket_end == bucket_begin) return PG_OK;
    hipLaunchKernelGGL(bucket_fill_kernel, dim3((unsigned)(bucket_end - bucket_begin)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)t->data + ((uint64_t)bucket_begin << t->log2_bucket_slots), t->log2_bucket_slots, (long long *)fill);
    return check_launch("pg_table_bucket_fill_range");
}

extern "C" int pg_table_compact_planes_range(const pg_table *t, int64_t bucket_begin, int64_t bucket_end, const int64_t *tag_elem,
                                             const int64_t *cnt_elem, void *out, uint64_t *overflow, uint64_t *overflow_count,
                                             int64_t overflow_cap, uint32_t *status, void *stream)
{
    int rc = check_bucketed(t, "pg_table_compact_planes_range");
    if (rc) return rc;
    const int bits = t->log2_slots - t->log2_bucket_slots;
    if (KEY_BITS - bits > 31) return pg_fail(PG_EINVAL, "pg_table_compact_planes_range: needs at least 2^11 buckets (tags of at most 31 bits)");
    if (!tag_elem || !cnt_elem || !out || !overflow || !overflow_count || !status || bucket_begin < 0 || bucket_end < bucket_begin ||
        bucket_end > ((int64_t)1 << bits))
        return pg_fail(PG_EINVAL, "pg_table_compact_planes_range: bad arguments");
    if (bucket_end == bucket_begin) return PG_OK;
    hipLaunchKernelGGL(table_compact_planes_kernel, dim3((unsigned)(bucket_end - bucket_begin)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)t->data + ((uint64_t)bucket_begin << t->log2_bucket_slots), t->log2_bucket_slots,
                       (const long long *)tag_elem, (const long long *)cnt_elem, (uint32_t)((1u << (KEY_BITS - bits)) - 1u), (uint32_t *)out,
                       (uint16_t *)out, overflow, (unsigned long long *)overflow_count, (unsigned long long)overflow_cap, status);
    return check_launch("pg_table_compact_planes_range");
}

extern "C" int pg_table_compact(const pg_table *t, const int64_t *seg, uint64_t *out, void *stream)
{
    int rc = check_bucketed(t, "pg_table_compact");
    if (rc) return rc;
    if (!seg || !out) return pg_fail(PG_EINVAL, "pg_table_compact: null argument");
    hipLaunchKernelGGL(table_compact_kernel, dim3(1u << (t->log2_slots - t->log2_bucket_slots)), dim3(BLOCK), 0, (hipStream_t)stream,
                       (const uint64_t *)t->data, t->log2_bucket_slots, (const long long *)seg, out);
    return check_launch("pg_table_compact");
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
    const HashView v = t->kind == PG_TABLE_DENSE ? HashView{nullptr, 0, 0} : view_of(t);
    const uint32_t *dense = t->kind == PG_TABLE_DENSE ? (const uint32_t *)t->data : nullptr;
#define PG_LAUNCH(TK) hipLaunchKernelGGL((table_query_kernel<TK>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, codes, n, t->k, dense, v, counts)
    switch (t->kind) {
    case PG_TABLE_DENSE: PG_LAUNCH(TK_DENSE); break;
    case PG_TABLE_HASH: PG_LAUNCH(TK_HASH); break;
    case PG_TABLE_WIDE: PG_LAUNCH(TK_WIDE); break;
    case PG_TABLE_MINI: PG_LAUNCH(TK_MINI); break;
    default: PG_LAUNCH(TK_MINIW); break;
    }
#undef PG_LAUNCH
    return check_launch("pg_table_query");
}

extern "C" int pg_table_spectrum(const pg_table *t, int high, uint64_t *hist, void *stream)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_spectrum: t is null");
    if (!hist) return pg_fail(PG_EINVAL, "pg_table_spectrum: hist is null");
    if (high < 1 || high > PG_SPECTRUM_MAX_HIGH) return pg_fail(PG_EINVAL, "pg_table_spectrum: high %d outside [1, %d]", high, PG_SPECTRUM_MAX_HIGH);
    int rc = check_table(t);
    if (rc) return rc;
    if ((uintptr_t)t->data & 15) return pg_fail(PG_EINVAL, "pg_table_spectrum: t->data is not 16-byte aligned");
    // units of 16 bytes of the slots (planes form: 32 bytes of keys + 16 of counts); every form's table is a whole number of them
    int form;
    int64_t n_units;
    const uint4 *counts = nullptr;
    if (t->kind == PG_TABLE_DENSE) {
        form = SPEC_DENSE;
        n_units = (int64_t)1 << (2 * t->k - 2);
    } else if (t->kind == PG_TABLE_HASH || t->kind == PG_TABLE_MINI) {
        form = SPEC_PACKED;
        n_units = (int64_t)1 << (t->log2_slots - 1);
    } else {
        form = SPEC_PLANES;
        n_units = (int64_t)1 << (t->log2_slots - 2);
        counts = (const uint4 *)((const uint64_t *)t->data + ((int64_t)1 << t->log2_slots));
    }
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
#define PG_LAUNCH(FORM, BALLOT)                                                                                             \
    hipLaunchKernelGGL((table_spectrum_kernel<FORM, BALLOT>), dim3((unsigned)grid), dim3(BIG_BLOCK), lds, s, (const uint4 *)t->data, counts, n_units, \
                       high, (unsigned long long *)hist)
#define PG_LAUNCH_FORM(FORM)                                                                                                \
    do {                                                                                                                    \
        if (ballot <= 0) PG_LAUNCH(FORM, 0);                                                                                \
        else if (ballot == 1) PG_LAUNCH(FORM, 1);                                                                           \
        else PG_LAUNCH(FORM, 2);                                                                                            \
    } while (0)
    if (form == SPEC_DENSE) PG_LAUNCH_FORM(SPEC_DENSE);
    else if (form == SPEC_PACKED) PG_LAUNCH_FORM(SPEC_PACKED);
    else PG_LAUNCH_FORM(SPEC_PLANES);
#undef PG_LAUNCH_FORM
#undef PG_LAUNCH
    return check_launch("pg_table_spectrum");
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
    const HashView v = t->kind == PG_TABLE_DENSE ? HashView{nullptr, 0, 0} : view_of(t);
    const uint32_t *dense = t->kind == PG_TABLE_DENSE ? (const uint32_t *)t->data : nullptr;
#define PG_LAUNCH(TK)                                                                                                          \
    hipLaunchKernelGGL((table_profile_kernel<TK>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, codes, valid, n_chars, char_begin, n, \
                       t->k, dense, v, counts)
    switch (t->kind) {
    case PG_TABLE_DENSE: PG_LAUNCH(TK_DENSE); break;
    case PG_TABLE_HASH: PG_LAUNCH(TK_HASH); break;
    case PG_TABLE_WIDE: PG_LAUNCH(TK_WIDE); break;
    case PG_TABLE_MINI: PG_LAUNCH(TK_MINI); break;
    default: PG_LAUNCH(TK_MINIW); break;
    }
#undef PG_LAUNCH
    return check_launch("pg_table_profile");
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
    const HashView v = t->kind == PG_TABLE_DENSE ? HashView{nullptr, 0, 0} : view_of(t);
    const uint32_t *dense = t->kind == PG_TABLE_DENSE ? (const uint32_t *)t->data : nullptr;
    const int grid = grid_for(n_ranges, WAVES);
    // room for one long range at least?  (a caller whose ranges are all short gives the head alone: two launches less)
    const int64_t room = (ws_bytes - DEPTH_HEAD_BYTES) / 4;
    const bool any_long = ws_bytes - DEPTH_HEAD_BYTES >= (int64_t)sizeof(DepthLong) + 4 * (PG_DEPTH_SHORT_MAX + 2 - PG_WIDE_MAX_K);
    const int fill_grid = grid_for((room + DEPTH_BATCH - 1) / DEPTH_BATCH);
    int64_t select_grid = (ws_bytes - DEPTH_HEAD_BYTES) / ((int64_t)sizeof(DepthLong) + 4 * (PG_DEPTH_SHORT_MAX + 2 - PG_WIDE_MAX_K));
    if (select_grid > 2048) select_grid = 2048;
#define PG_LAUNCH(TK)                                                                                                          \
    do {                                                                                                                       \
        hipLaunchKernelGGL((depth_short_kernel<TK>), dim3(grid), dim3(BLOCK), 0, s, codes, valid, n_chars, range_start, range_end, n_ranges, \
                           t->k, (uint64_t)lower, dense, v, (long long *)out, workspace, ws_bytes, status);                    \
        if (any_long)                                                                                                          \
            hipLaunchKernelGGL((depth_fill_kernel<TK>), dim3(fill_grid), dim3(BLOCK), 0, s, codes, valid, n_chars, (const void *)workspace, \
                               ws_bytes, t->k, dense, v, (const uint32_t *)status);                                            \
    } while (0)
    switch (t->kind) {
    case PG_TABLE_DENSE: PG_LAUNCH(TK_DENSE); break;
    case PG_TABLE_HASH: PG_LAUNCH(TK_HASH); break;
    case PG_TABLE_WIDE: PG_LAUNCH(TK_WIDE); break;
    case PG_TABLE_MINI: PG_LAUNCH(TK_MINI); break;
    default: PG_LAUNCH(TK_MINIW); break;
    }
#undef PG_LAUNCH
    if (any_long)
        hipLaunchKernelGGL(depth_select_kernel, dim3((unsigned)select_grid), dim3(BIG_BLOCK), 0, s, (const void *)workspace, ws_bytes,
                           (uint64_t)lower, (long long *)out, (const uint32_t *)status);
    return check_launch("pg_table_depth");
}

// the table as the dump kernels see it: form, entries, the counts plane of the planes form
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

extern "C" int64_t pg_table_dump_units(const pg_table *t)
{
    if (!t) return pg_fail(PG_EINVAL, "pg_table_dump_units: t is null");
    DumpView v;
    int rc = dump_view(t, "pg_table_dump_units", &v);
    if (rc) return rc;
    return (v.n_entries + PG_DUMP_UNIT_SLOTS - 1) / PG_DUMP_UNIT_SLOTS;
}

#define PG_DUMP_BY_FORM(form, LAUNCH)                                     \
    do {                                                                  \
        if ((form) == DUMP_DENSE) LAUNCH(DUMP_DENSE);                     \
        else if ((form) == DUMP_HASH) LAUNCH(DUMP_HASH);                  \
        else if ((form) == DUMP_MINI) LAUNCH(DUMP_MINI);                  \
        else LAUNCH(DUMP_PLANES);                                         \
    } while (0)

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
#define PG_LAUNCH(FORM)                                                                                                            \
    hipLaunchKernelGGL((table_dump_sizes_kernel<FORM>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const uint4 *)t->data, v.counts, \
                       v.n_entries, n_units, t->k, (uint64_t)lower, (long long *)unit_bytes, (long long *)unit_lines)
    PG_DUMP_BY_FORM(v.form, PG_LAUNCH);
#undef PG_LAUNCH
    return check_launch("pg_table_dump_sizes");
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
#define PG_LAUNCH(FORM)                                                                                                           \
    hipLaunchKernelGGL((table_dump_text_kernel<FORM>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const uint4 *)t->data, v.counts, \
                       v.n_entries, unit_begin, unit_end, t->k, (uint64_t)lower, (const long long *)unit_offsets, text_base, range_bytes, text)
    PG_DUMP_BY_FORM(v.form, PG_LAUNCH);
#undef PG_LAUNCH
    return check_launch("pg_table_dump_text");
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
    const void *fn = mini ? (const void *)table_merge_aligned_kernel<true> : (const void *)table_merge_aligned_kernel<false>;
    if ((rc = raise_lds_limit(fn, lds, "pg_table_merge_aligned"))) return rc;
    if (mini)
        hipLaunchKernelGGL((table_merge_aligned_kernel<true>), dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, ms, n_srcs, view_of(dst), status);
    else
        hipLaunchKernelGGL((table_merge_aligned_kernel<false>), dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, ms, n_srcs, view_of(dst), status);
    return check_launch("pg_table_merge_aligned");
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
    const HashView t = dst->kind == PG_TABLE_DENSE ? HashView{nullptr, 0, 0} : view_of(dst);
    uint32_t *dense = dst->kind == PG_TABLE_DENSE ? (uint32_t *)dst->data : nullptr;
#define PG_LAUNCH_TO(FORM, TK)                                                                                                     \
    hipLaunchKernelGGL((table_merge_kernel<FORM, TK>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const uint4 *)src->data, v.counts, \
                       n_quads, dst->k, dense, t, status)
#define PG_LAUNCH(FORM)                                                   \
    do {                                                                  \
        switch (dst->kind) {                                              \
        case PG_TABLE_DENSE: PG_LAUNCH_TO(FORM, TK_DENSE); break;         \
        case PG_TABLE_HASH: PG_LAUNCH_TO(FORM, TK_HASH); break;           \
        case PG_TABLE_WIDE: PG_LAUNCH_TO(FORM, TK_WIDE); break;           \
        case PG_TABLE_MINI: PG_LAUNCH_TO(FORM, TK_MINI); break;           \
        default: PG_LAUNCH_TO(FORM, TK_MINIW); break;                     \
        }                                                                 \
    } while (0)
    PG_DUMP_BY_FORM(v.form, PG_LAUNCH);
#undef PG_LAUNCH
#undef PG_LAUNCH_TO
    return check_launch("pg_table_merge");
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
    const void *fn = mini ? (const void *)table_combine_aligned_kernel<true> : (const void *)table_combine_aligned_kernel<false>;
    if ((rc = raise_lds_limit(fn, lds, who))) return rc;
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
    const ulonglong2 *pa = (const ulonglong2 *)a->data, *pb = b ? (const ulonglong2 *)b->data : nullptr;
    if (mini)
        hipLaunchKernelGGL((table_combine_aligned_kernel<true>), dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, pa, pb, op, (uint64_t)lower,
                           up, view_of(dst), status);
    else
        hipLaunchKernelGGL((table_combine_aligned_kernel<false>), dim3(1u << bits), dim3(BIG_BLOCK), lds, (hipStream_t)stream, pa, pb, op, (uint64_t)lower,
                           up, view_of(dst), status);
    return check_launch(who);
}

// the probed table of the general form and of the comparison: kernel by (form of a, kind of b; TK_NONE: no b)
#define PG_COMBINE_BY_KIND(FORM, b, LAUNCH)                               \
    do {                                                                  \
        if (!(b)) LAUNCH(FORM, TK_NONE);                                  \
        else switch ((b)->kind) {                                         \
        case PG_TABLE_DENSE: LAUNCH(FORM, TK_DENSE); break;               \
        case PG_TABLE_HASH: LAUNCH(FORM, TK_HASH); break;                 \
        case PG_TABLE_WIDE: LAUNCH(FORM, TK_WIDE); break;                 \
        case PG_TABLE_MINI: LAUNCH(FORM, TK_MINI); break;                 \
        default: LAUNCH(FORM, TK_MINIW); break;                           \
        }                                                                 \
    } while (0)

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
    const HashView hb = !b || b->kind == PG_TABLE_DENSE ? HashView{nullptr, 0, 0} : view_of(b);
    const uint32_t *dense_b = b && b->kind == PG_TABLE_DENSE ? (const uint32_t *)b->data : nullptr;
    const uint64_t up = upper < 0 ? ~0ull : (uint64_t)upper;
#define PG_LAUNCH_ON(FORM, TK)                                                                                                     \
    hipLaunchKernelGGL((table_combine_items_kernel<FORM, TK>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const uint4 *)a->data, v.counts, \
                       n_quads, a->k, dense_b, hb, op, (uint64_t)lower, up, codes, counts, (unsigned long long)cap, (unsigned long long *)n_out, status)
#define PG_LAUNCH(FORM) PG_COMBINE_BY_KIND(FORM, b, PG_LAUNCH_ON)
    PG_DUMP_BY_FORM(v.form, PG_LAUNCH);
#undef PG_LAUNCH
#undef PG_LAUNCH_ON
    return check_launch(who);
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
    const HashView hb = !b || b->kind == PG_TABLE_DENSE ? HashView{nullptr, 0, 0} : view_of(b);
    const uint32_t *dense_b = b && b->kind == PG_TABLE_DENSE ? (const uint32_t *)b->data : nullptr;
    if (hipMemsetAsync(out, 0, 4 * sizeof(uint64_t), (hipStream_t)stream) != hipSuccess) return pg_fail(PG_EHIP, "%s: cannot clear out", who);
#define PG_LAUNCH_ON(FORM, TK)                                                                                                     \
    hipLaunchKernelGGL((table_compare_kernel<FORM, TK>), dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const uint4 *)a->data, v.counts, n_quads, \
                       a->k, dense_b, hb, (unsigned long long *)out)
#define PG_LAUNCH(FORM) PG_COMBINE_BY_KIND(FORM, b, PG_LAUNCH_ON)
    PG_DUMP_BY_FORM(v.form, PG_LAUNCH);
#undef PG_LAUNCH
#undef PG_LAUNCH_ON
    return check_launch(who);
}
#undef PG_COMBINE_BY_KIND
#undef PG_DUMP_BY_FORM

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

extern "C" int64_t pg_abundance_workspace_bytes(int64_t n_words_counted, int64_t n_rows, int vsize, const pg_table *t)
{
    if (n_words_counted < 0 || n_rows < 0) return pg_fail(PG_EINVAL, "negative size");
    int rc = check_table(t);
    if (rc) return rc;
    BucketPlan p;
    if ((rc = plan_buckets(t, n_words_counted, &p))) return rc;
    ShufflePlan sp;
    if ((rc = plan_shuffle(p.cap, n_rows, vsize, (int64_t)1 << p.bits, &sp))) return rc;
    return (int64_t)sp.total;
}

static int abundance_impl(const pg_table *t, const pg_rows *rows, int window, int vsize, int32_t *abd_out,
                          const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                          void *workspace, int64_t workspace_bytes, void *stream, bool emitted);
static int shuffle_tail(const ShufflePlan &sp, const unsigned long long *in_begin, int nb, const pg_rows *rows, int vsize,
                        int32_t *abd_out, char *ws, hipStream_t s);

// for the other translation units (pg_internal.h): where the lookup pass of another pipeline leaves its words, and the
// row shuffle that finishes them
int pg_internal_shuffle_layout(int64_t cap, int64_t n_rows, int vsize, pg_shuffle_layout *out, int one_pass_bits, int no_input)
{
    ShufflePlan sp;
    int rc = plan_shuffle(cap, n_rows, vsize, 0, &sp, one_pass_bits, no_input);
    if (rc) return rc;
    out->vbits = sp.vbits;
    out->emit_off = sp.emit_off;
    out->words_e_off = sp.words_e_off;
    out->words_a_off = sp.words_a_off;
    out->total = sp.total;
    return PG_OK;
}

int pg_internal_shuffle_rows(const unsigned long long *in_begin, int nb, int64_t cap, const pg_rows *rows, int vsize, int32_t *abd_out,
                             void *workspace, int64_t workspace_bytes, void *stream)
{
    ShufflePlan sp;
    int rc = plan_shuffle(cap, rows->n_rows, vsize, 0, &sp);
    if (rc) return rc;
    if ((int64_t)sp.total > workspace_bytes) return pg_fail(PG_EINVAL, "row shuffle: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)sp.total);
    if (rows->n_rows == 0) return PG_OK;
    return shuffle_tail(sp, in_begin, nb, rows, vsize, abd_out, (char *)workspace, (hipStream_t)stream);
}

extern "C" int pg_abundance_from_records(const pg_table *t, const pg_rows *rows, int window, int vsize, int32_t *abd_out,
                                         const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                                         void *workspace, int64_t workspace_bytes, void *stream)
{
    return abundance_impl(t, rows, window, vsize, abd_out, count_workspace, count_workspace_bytes, n_words_counted, workspace, workspace_bytes,
                          stream, false);
}

extern "C" int pg_abundance_from_emitted(const pg_table *t, const pg_rows *rows, int window, int vsize, int32_t *abd_out,
                                         const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                                         void *workspace, int64_t workspace_bytes, void *stream)
{
    return abundance_impl(t, rows, window, vsize, abd_out, count_workspace, count_workspace_bytes, n_words_counted, workspace, workspace_bytes,
                          stream, true);
}

static int abundance_impl(const pg_table *t, const pg_rows *rows, int window, int vsize, int32_t *abd_out,
                          const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                          void *workspace, int64_t workspace_bytes, void *stream, bool emitted)
{
    int rc = check_table(t);
    if (rc) return rc;
    if (!rows || !abd_out || !count_workspace || !workspace) return pg_fail(PG_EINVAL, "pg_abundance_from_records: null argument");
    if ((rc = check_rows(rows, "pg_abundance_from_records"))) return rc;
    if (window < 1) return pg_fail(PG_EINVAL, "pg_abundance_from_records: window %d", window);
    if ((int64_t)window * vsize > (int64_t)PG_HASH_COUNT_SAT)
        return pg_fail(PG_EINVAL, "pg_abundance_from_records: window*vector_size %lld exceeds the exact range of the hash table (%u)",
                       (long long)window * vsize, PG_HASH_COUNT_SAT);
    BucketPlan p;
    if ((rc = plan_buckets(t, n_words_counted, &p))) return rc;
    if ((int64_t)p.total > count_workspace_bytes) return pg_fail(PG_EINVAL, "pg_abundance_from_records: count workspace does not match n_words_counted");
    ShufflePlan sp;
    if ((rc = plan_shuffle(p.cap, rows->n_rows, vsize, (int64_t)1 << p.bits, &sp))) return rc;
    if ((int64_t)sp.total > workspace_bytes)
        return pg_fail(PG_EINVAL, "pg_abundance_from_records: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)sp.total);
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) return pg_fail(PG_EINVAL, "pg_abundance_from_records: workspace must be 256-byte aligned");
    if (rows->n_rows == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    const char *cws = (const char *)count_workspace;
    const auto *off = (const unsigned long long *)(cws + p.off_off);
    const auto *recs = (const uint64_t *)(cws + p.final_off());
    char *ws = (char *)workspace;
    auto *emit_end = (unsigned long long *)(ws + sp.emit_off);
    auto *words_e = (uint32_t *)(ws + sp.words_e_off);
    const int nb = 1 << p.bits;
    const size_t slice_lds = (size_t)8 << t->log2_bucket_slots;
    if ((rc = raise_lds_limit((const void *)bucket_lookup_kernel, slice_lds, "pg_abundance_from_records"))) return rc;
    // (emitted: the lookup pass already ran inside pg_kmer_count_bucketed_emit and left emit_end + the words behind)
    if (!emitted && hipMemsetAsync(ws, 0, sp.caps_off, s) != hipSuccess)
        return pg_fail(PG_EHIP, "pg_abundance_from_records: memset failed");
    // S1: counts out of the LDS copies of the slices -> (row, bin) words, packed per bucket
    if (emitted) {
    } else if (KEY_BITS - p.bits <= 31 && !getenv("PG_B64")) {
        if ((rc = raise_lds_limit((const void *)bucket_lookup32_kernel, slice_lds, "pg_abundance_from_records"))) return rc;
        hipLaunchKernelGGL(bucket_lookup32_kernel, dim3(nb), dim3(BIG_BLOCK), slice_lds, s, recs, off, view_of(t), (uint32_t)window, (uint32_t)vsize,
                           sp.vbits, words_e, emit_end);
    } else
    hipLaunchKernelGGL(bucket_lookup_kernel, dim3(nb), dim3(BIG_BLOCK), slice_lds, s, recs, off, view_of(t), (uint32_t)window, (uint32_t)vsize, sp.vbits,
                       words_e, emit_end);
    return shuffle_tail(sp, off, nb, rows, vsize, abd_out, ws, s);
}

// S2 + S3: the (row, bin) words of every bucket b, words_e[in_begin[b] .. emit_end[b]), -> rows of the abundance matrix.
// Three parts so that a lookup pass which scatters its words by row group itself (mini.hip) can take the first pass's place:
//   prepare   row-group capacities -> offsets of the group regions, cursors cleared
//   pass one  scatter by the first gb1 bits of the row group
//   finish    the second pass (more than 2^10 groups only) and the LDS row histograms
static int shuffle_prepare(const ShufflePlan &sp, const pg_rows *rows, char *ws, hipStream_t s)
{
    auto *caps = (unsigned long long *)(ws + sp.caps_off);
    auto *goff = (unsigned long long *)(ws + sp.goff_off);
    if (hipMemsetAsync(ws + sp.caps_off, 0, sp.dhist_off - sp.caps_off, s) != hipSuccess)
        return pg_fail(PG_EHIP, "pg_abundance_from_records: memset failed");
    hipLaunchKernelGGL(group_caps_kernel, dim3((unsigned)((sp.n_groups_padded + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, rows->row_start, rows->row_end,
                       rows->n_rows, sp.n_groups_padded, caps);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)caps, sp.n_groups_padded, goff);
    return check_launch("pg_abundance_from_records");
}

static int shuffle_finish(const ShufflePlan &sp, const pg_rows *rows, int vsize, int32_t *abd_out, char *ws, hipStream_t s, int word_form = PG_SHUFFLE_WORDS_PLAIN)
{
    const bool narrow = word_form == PG_SHUFFLE_WORDS_NARROW, counted = word_form == PG_SHUFFLE_WORDS_COUNTED;
    if (counted && sp.vbits + GROUP_ROWS_LOG2 + sp.gbits > PG_SHUFFLE_COUNT_SHIFT) return pg_fail(PG_EINVAL, "row shuffle: counted words need row bits + bin bits <= %d", PG_SHUFFLE_COUNT_SHIFT);
    int rc;
    auto *goff = (unsigned long long *)(ws + sp.goff_off);
    auto *gcur1 = (unsigned long long *)(ws + sp.gcur1_off);
    auto *gcur2 = (unsigned long long *)(ws + sp.gcur2_off);
    auto *words_a = (uint32_t *)(ws + sp.words_a_off);
    auto *words_b = (uint32_t *)(ws + sp.words_b_off);
    const size_t hist_lds = ((size_t)4 << GROUP_ROWS_LOG2) * (size_t)(vsize | 1);
    if ((rc = raise_lds_limit((const void *)row_hist_kernel<uint32_t>, hist_lds, "pg_abundance_from_records"))) return rc;
    if ((rc = raise_lds_limit((const void *)row_hist_kernel<uint16_t>, hist_lds, "pg_abundance_from_records"))) return rc;
    if ((rc = raise_lds_limit((const void *)row_hist_kernel<uint32_t, true>, hist_lds, "pg_abundance_from_records"))) return rc;
    if (narrow && sp.gb2) return pg_fail(PG_EINVAL, "row shuffle: narrow words need a one-pass shuffle");
    const int gshift = sp.vbits + GROUP_ROWS_LOG2;
    const unsigned long long *gcnt = gcur1;
    const uint32_t *final_words = words_a;
    if (sp.gb2) {
        const int tiles_x = 64;
        hipLaunchKernelGGL((scatter_records_kernel<uint32_t, DIG_ROW, RPL32, MAX_FAN_BITS>), dim3((unsigned)(tiles_x << sp.gb1)), dim3(BLOCK), 0, s,
                           (const uint32_t *)words_a, (const unsigned long long *)goff, (const unsigned long long *)nullptr, sp.gb2,
                           (const unsigned long long *)gcur1, tiles_x, words_b, (const unsigned long long *)goff, gcur2, 0, 0, sp.gb2, gshift);
        gcnt = gcur2;
        final_words = words_b;
    }
    // S3: LDS row histograms -> rows of the matrix.  One workgroup per group and CU: the groups of a last round that would leave most
    // CUs idle (at most a quarter of them busy) are shared out instead, `split` workgroups each (PG_ROW_HIST_SPLIT="groups,split"
    // forces a split, "0" none)
    static int n_cus = 0;
    if (!n_cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cus <= 0) n_cus = 256;
    }
    int64_t n_tail = sp.n_groups > n_cus ? sp.n_groups % n_cus : 0;
    int split = n_tail > 0 && n_tail <= n_cus / 4 ? (int)std::min<int64_t>(32, n_cus / n_tail) : 1;
    if (const char *force = getenv("PG_ROW_HIST_SPLIT")) {
        long long fg = 0, fs = 1;
        if (sscanf(force, "%lld,%lld", &fg, &fs) == 2 && fg > 0 && fs > 1) { n_tail = std::min<int64_t>(fg, sp.n_groups); split = (int)std::min<long long>(fs, 64); }
        else { n_tail = 0; split = 1; }
    }
    if (split <= 1) n_tail = 0;
    const int64_t n_main = sp.n_groups - n_tail;
    if (n_tail) {
        const int64_t row0 = n_main << GROUP_ROWS_LOG2;
        if (row0 < rows->n_rows && hipMemsetAsync(abd_out + row0 * (int64_t)vsize, 0, (size_t)(rows->n_rows - row0) * vsize * sizeof(int32_t), s) != hipSuccess)
            return pg_fail(PG_EHIP, "pg_abundance_from_records: memset failed");
    }
#define PG_ROW_HIST(WORD_, COUNTED_, WORDS_)                                                                                 \
    do {                                                                                                                    \
        if (n_main) hipLaunchKernelGGL((row_hist_kernel<WORD_, COUNTED_>), dim3((unsigned)n_main), dim3(BIG_BLOCK), hist_lds, s, WORDS_, (const unsigned long long *)goff, \
                                       gcnt, sp.vbits, (uint32_t)vsize, rows->n_rows, abd_out, (int64_t)0, 1);               \
        if (n_tail) hipLaunchKernelGGL((row_hist_kernel<WORD_, COUNTED_>), dim3((unsigned)(n_tail * split)), dim3(BIG_BLOCK), hist_lds, s, WORDS_,           \
                                       (const unsigned long long *)goff, gcnt, sp.vbits, (uint32_t)vsize, rows->n_rows, abd_out, n_main, split); \
    } while (0)
    if (narrow) PG_ROW_HIST(uint16_t, false, (const uint16_t *)final_words);
    else if (counted) PG_ROW_HIST(uint32_t, true, final_words);
    else PG_ROW_HIST(uint32_t, false, final_words);
#undef PG_ROW_HIST
    return check_launch("pg_abundance_from_records");
}

static int shuffle_tail(const ShufflePlan &sp, const unsigned long long *in_begin, int nb, const pg_rows *rows, int vsize,
                        int32_t *abd_out, char *ws, hipStream_t s)
{
    int rc = shuffle_prepare(sp, rows, ws, s);
    if (rc) return rc;
    auto *emit_end = (unsigned long long *)(ws + sp.emit_off);
    auto *goff = (unsigned long long *)(ws + sp.goff_off);
    auto *gcur1 = (unsigned long long *)(ws + sp.gcur1_off);
    auto *words_e = (uint32_t *)(ws + sp.words_e_off);
    auto *words_a = (uint32_t *)(ws + sp.words_a_off);
    const unsigned long long *off = in_begin;
    const int gshift = sp.vbits + GROUP_ROWS_LOG2;
    // S2a: scatter the words by the first gb1 bits of their row group (destinations from global cursors, one add per digit
    // and tile)
    {
        // ONE workgroup per bucket walks the bucket's tiles (about five wide ones): measured 10.5 ms against 12.2 / 13.8 / 14.9 ms with
        // 2 / 4 / 8 workgroups per bucket -- every workgroup first waits for the two dependent loads of its region bounds
        const int tiles_x = 1;
        if (sp.gb1 > MAX_FAN_BITS)         // all row groups in ONE pass: bigger tiles keep the runs per group at 64 B
            hipLaunchKernelGGL((scatter_records_kernel<uint32_t, DIG_ROW, RPL32_WIDE, WIDE_FAN_BITS>), dim3((unsigned)(tiles_x * nb)), dim3(BLOCK), 0, s,
                               (const uint32_t *)words_e, off, (const unsigned long long *)emit_end, 0, (const unsigned long long *)nullptr, tiles_x,
                               words_a, (const unsigned long long *)goff, gcur1, sp.gb2, 1, sp.gb1, gshift + sp.gb2);
        else
        hipLaunchKernelGGL((scatter_records_kernel<uint32_t, DIG_ROW, RPL32, MAX_FAN_BITS>), dim3((unsigned)(tiles_x * nb)), dim3(BLOCK), 0, s,
                           (const uint32_t *)words_e, off, (const unsigned long long *)emit_end, 0, (const unsigned long long *)nullptr, tiles_x,
                           words_a, (const unsigned long long *)goff, gcur1, sp.gb2, 1, sp.gb1, gshift + sp.gb2);
    }
    return shuffle_finish(sp, rows, vsize, abd_out, ws, s);
}

// the two outer parts for a lookup pass that does the first scatter itself: `ctx` tells it where the group regions are
int pg_internal_shuffle_is_narrow(int64_t cap, int64_t n_rows, int vsize, int one_pass_bits)
{
    ShufflePlan sp;
    if (plan_shuffle(cap, n_rows, vsize, 0, &sp, one_pass_bits)) return 0;
    return sp.gb2 == 0 && sp.vbits + GROUP_ROWS_LOG2 <= 15 && !getenv("PG_WIDE_WORDS");
}

int pg_internal_shuffle_prepare(int64_t cap, const pg_rows *rows, int vsize, void *workspace, int64_t workspace_bytes, void *stream,
                                pg_shuffle_ctx *ctx, int one_pass_bits, int no_input, int ctx_only)
{
    ShufflePlan sp;
    int rc = plan_shuffle(cap, rows->n_rows, vsize, 0, &sp, one_pass_bits, no_input);
    if (rc) return rc;
    if ((int64_t)sp.total > workspace_bytes) return pg_fail(PG_EINVAL, "row shuffle: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)sp.total);
    char *ws = (char *)workspace;
    ctx->goff = (const unsigned long long *)(ws + sp.goff_off);
    ctx->gcur1 = (unsigned long long *)(ws + sp.gcur1_off);
    ctx->words_in = (uint32_t *)(ws + sp.words_e_off);
    ctx->words_out = (uint32_t *)(ws + sp.words_a_off);
    ctx->vbits = sp.vbits;
    ctx->gb1 = sp.gb1;
    ctx->gb2 = sp.gb2;
    ctx->dshift = sp.vbits + GROUP_ROWS_LOG2 + sp.gb2;
    ctx->narrow = pg_internal_shuffle_is_narrow(cap, rows->n_rows, vsize, one_pass_bits);
    ctx->words_cap = (unsigned long long)cap;
    if (rows->n_rows == 0 || ctx_only) return PG_OK;             // (ctx_only: offsets and cursors are in use already -- a further launch into them)
    return shuffle_prepare(sp, rows, ws, (hipStream_t)stream);
}

int pg_internal_shuffle_finish(int64_t cap, const pg_rows *rows, int vsize, int32_t *abd_out, void *workspace, int64_t workspace_bytes, void *stream,
                               int word_form, int one_pass_bits, int no_input)
{
    ShufflePlan sp;
    int rc = plan_shuffle(cap, rows->n_rows, vsize, 0, &sp, one_pass_bits, no_input);
    if (rc) return rc;
    if ((int64_t)sp.total > workspace_bytes) return pg_fail(PG_EINVAL, "row shuffle: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)sp.total);
    if (rows->n_rows == 0) return PG_OK;
    return shuffle_finish(sp, rows, vsize, abd_out, (char *)workspace, (hipStream_t)stream, word_form);
}

// a9: L1 row normalisation in float64, narrowed to float32, + the sampling weight; one wavefront per row (src/data.py:16-21)
namespace {
__global__ __launch_bounds__(BLOCK) void normalize_rows_kernel(const int32_t *__restrict__ m, int64_t n_rows, int n_cols,
                                                               float *__restrict__ out, double *__restrict__ weight)
{
    const int64_t r = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (r >= n_rows) return;
    const uint32_t lane = threadIdx.x & 63;
    const int32_t *row = m + r * n_cols;
    long long sum = 0;
    int32_t top = INT32_MIN;
    for (int c = lane; c < n_cols; c += 64) {
        const int32_t x = row[c];
        sum += x < 0 ? -(long long)x : (long long)x;
        top = x > top ? x : top;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d);
        const int32_t o = __shfl_xor(top, d);
        top = o > top ? o : top;
    }
    const double norm = sum == 0 ? 1.0 : (double)sum;                // (sklearn: a zero norm counts as 1)
    float *dst = out + r * n_cols;
    for (int c = lane; c < n_cols; c += 64) dst[c] = (float)((double)row[c] / norm);
    if (weight && lane == 0) {
        const double q = n_cols > 0 ? (double)top / norm : 0.0;
        weight[r] = q * q;
    }
}
}  // namespace

extern "C" int pg_normalize_rows(const int32_t *m, int64_t n_rows, int n_cols, float *out, double *weight, void *stream)
{
    if (n_rows < 0 || n_cols < 0) return pg_fail(PG_EINVAL, "pg_normalize_rows: negative size");
    if (n_rows == 0 || n_cols == 0) return PG_OK;
    if (!m || !out) return pg_fail(PG_EINVAL, "pg_normalize_rows: null argument");
    const int64_t per = BLOCK / 64;
    const int64_t grid = (n_rows + per - 1) / per;
    if (grid > 0x7fffffffLL) return pg_fail(PG_EINVAL, "pg_normalize_rows: too many rows for one launch");
    hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)grid), dim3(BLOCK), 0, (hipStream_t)stream, m, n_rows, n_cols, out, weight);
    return check_launch("pg_normalize_rows");
}

extern "C" int pg_features(const uint64_t *codes, const uint32_t *valid, int64_t n_words,
                           const int32_t *seg_row, const int64_t *seg_start, const int64_t *seg_end, int64_t n_segs,
                           int k_tnf, const uint16_t *colmap, int32_t *tnf_out,
                           const pg_table *t, int window, int vsize, int32_t *abd_out, void *stream)
{
    if (!codes || !valid || n_words < 0) return pg_fail(PG_EINVAL, "pg_features: null stream arrays");
    if (n_segs < 0 || (n_segs > 0 && (!seg_row || !seg_start || !seg_end))) return pg_fail(PG_EINVAL, "pg_features: bad segment arrays");
    if (n_segs > 0x7fffffffLL) return pg_fail(PG_EINVAL, "pg_features: too many segments for one launch");
    const bool do_tnf = tnf_out != nullptr;
    const bool do_abd = abd_out != nullptr;
    if (!do_tnf && !do_abd) return pg_fail(PG_EINVAL, "pg_features: no output requested");
    int tnf_cols = 0, tnf_copies = 0, n_raw = 0;
    if (do_tnf) {
        if (k_tnf < 1 || k_tnf > PG_TNF_MAX_K) return pg_fail(PG_EINVAL, "pg_features: tnf k must be in [1,%d] (got %d)", PG_TNF_MAX_K, k_tnf);
        if (!colmap) return pg_fail(PG_EINVAL, "pg_features: colmap is null");
        tnf_cols = pg_tnf_ncols(k_tnf);
        n_raw = 1 << (2 * k_tnf);
        tnf_copies = k_tnf <= 4 ? WAVES : 1;
    }
    int kind = TK_NONE, k = 0;
    HashView view{nullptr, 0, 0};
    const uint32_t *dense = nullptr;
    if (do_abd) {
        int rc = check_table(t);
        if (rc) return rc;
        if (window < 1 || vsize < 1 || vsize > 8192) return pg_fail(PG_EINVAL, "pg_features: window %d / vector size %d out of range", window, vsize);
        if ((t->kind == PG_TABLE_HASH || t->kind == PG_TABLE_MINI) && (int64_t)window * vsize > (int64_t)PG_HASH_COUNT_SAT)
            return pg_fail(PG_EINVAL, "pg_features: window*vector_size %lld exceeds the exact range of the hash table (%u)",
                           (long long)window * vsize, PG_HASH_COUNT_SAT);
        kind = t->kind == PG_TABLE_DENSE ? TK_DENSE : t->kind == PG_TABLE_WIDE ? TK_WIDE : t->kind == PG_TABLE_MINI ? TK_MINI
             : t->kind == PG_TABLE_MINI_WIDE ? TK_MINIW : TK_HASH;
        k = t->k;
        if (kind == TK_DENSE) dense = (const uint32_t *)t->data;
        else view = view_of(t);
    }
    if (n_segs == 0) return PG_OK;
    const int abd_copies = do_abd ? (vsize <= 1024 ? WAVES : 1) : 0;
    const size_t lds_bytes = sizeof(uint32_t) * ((size_t)abd_copies * (do_abd ? vsize : 0) + (size_t)tnf_copies * n_raw);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)n_segs), block(BLOCK);
#define PG_LAUNCH(KT, TK)                                                                                                   \
    hipLaunchKernelGGL((features_kernel<KT, TK>), grid, block, lds_bytes, s, codes, valid, n_words, seg_row, seg_start, seg_end, \
                       k_tnf, colmap, tnf_cols, tnf_copies, abd_copies, tnf_out, k, dense, view, (uint32_t)window, vsize, abd_out)
    if (kind == TK_NONE) PG_LAUNCH(uint32_t, TK_NONE);
    else if (kind == TK_DENSE) PG_LAUNCH(uint32_t, TK_DENSE);
    else if (kind == TK_WIDE) PG_LAUNCH(uint64_t, TK_WIDE);
    else if (kind == TK_MINI) PG_LAUNCH(uint64_t, TK_MINI);
    else if (kind == TK_MINIW) PG_LAUNCH(uint64_t, TK_MINIW);
    else PG_LAUNCH(uint64_t, TK_HASH);
#undef PG_LAUNCH
    return check_launch("pg_features");
}
