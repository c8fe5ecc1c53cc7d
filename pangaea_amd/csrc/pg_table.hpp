// pg_table.hpp -- the k-mer table as device and host code see it, shared by kernels.hip (which builds tables and reads them on
// the timed path) and table_ops.hip (every operation on a finished table): the kinds, the view of a hash table, its probes and
// inserts, the lookup in two halves, and the host-side checks and kind dispatch.  An anonymous namespace, as pg_device.hpp: each
// translation unit gets its own copy.
#ifndef PG_TABLE_HPP
#define PG_TABLE_HPP
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

// the inserts below report a table without room as kmer_merge_kernel always has: bit 0 of the status word
static_assert(PG_STATUS_TABLE_FULL == 1u, "PG_STATUS_TABLE_FULL is the 1u the count kernels write");

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

// One lookup in two halves, so that a lane issues the first probes of a batch before it resolves any: issue() derives key and home
// slot by the table's kind and starts the first read, resolve() answers the stored count (0: not there).  TK_NONE (no table) answers
// 0 without a read.  The dense kind is indexed by the code: a caller whose code comes from another table checks it against 4^k.
template <int TK> struct Lookup {
    uint64_t key, hh, cur;
    // (issue_key: the caller has the table's key already -- the key42 of a packed hash table, the code itself for every other kind)
    __device__ __forceinline__ void issue_key(uint64_t canon, uint64_t key_, int k, const uint32_t *__restrict__ dense, const HashView &t)
    {
        if (TK == TK_NONE) return;
        if (TK == TK_DENSE) {
            cur = dense[(uint32_t)canon];
            return;
        }
        key = key_;
        hh = TK == TK_WIDE ? t.home_wide(canon) : (TK == TK_MINI || TK == TK_MINIW) ? t.home_mini(canon, k) : t.home_key(key);
        cur = t.slots[hh];
    }
    __device__ __forceinline__ void issue(uint64_t canon, int k, const uint32_t *__restrict__ dense, const HashView &t)
    {
        issue_key(canon, TK == TK_HASH ? key42(canon) : canon, k, dense, t);
    }
    __device__ __forceinline__ uint32_t resolve(const HashView &t) const
    {
        bool found;
        if (TK == TK_NONE) return 0u;
        if (TK == TK_DENSE) return (uint32_t)cur;
        if (TK == TK_WIDE || TK == TK_MINIW) return wide_probe(t, hh, cur, key, &found);
        return hash_probe(t, hh, cur, key, &found);
    }
};

// merge into a table held in LDS (bucket_merge_kernel of kernels.hip, the aligned kernels of table_ops.hip)
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

// -------------------------------------------------------------------------------- host side
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


// what a probing kernel takes of a table (null: no table): the counters of the dense kind, the view of every other
struct ProbeArgs {
    uint32_t *dense;
    HashView view;
};
__attribute__((unused)) ProbeArgs probe_args(const pg_table *t)
{
    if (!t) return {nullptr, HashView{nullptr, 0, 0}};
    return t->kind == PG_TABLE_DENSE ? ProbeArgs{(uint32_t *)t->data, HashView{nullptr, 0, 0}} : ProbeArgs{nullptr, view_of(t)};
}

// kernel by the kind of a checked table (typed dispatch, pg_device.hpp): f(int_tag<TK_DENSE | TK_HASH | TK_WIDE | TK_MINI | TK_MINIW>)
template <class F> int with_kind(int kind, F &&f)
{
    switch (kind) {
    case PG_TABLE_DENSE: return f(int_tag<TK_DENSE>{});
    case PG_TABLE_HASH: return f(int_tag<TK_HASH>{});
    case PG_TABLE_WIDE: return f(int_tag<TK_WIDE>{});
    case PG_TABLE_MINI: return f(int_tag<TK_MINI>{});
    default: return f(int_tag<TK_MINIW>{});
    }
}
// ... of a table that may be absent: f(int_tag<TK_NONE>) for null
template <class F> int with_kind_or_none(const pg_table *t, F &&f) { return t ? with_kind(t->kind, f) : f(int_tag<TK_NONE>{}); }

}  // namespace
#endif
