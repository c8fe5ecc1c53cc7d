// mini.hip -- the super-k-mer form of K2 (global multiplicities) with K3's lookups inside, for PG_TABLE_MINI tables.
//
// Replaces (reference file:line, /root/reference/src): jellyfish count -C (feature.py:94) + the dump reload of
// cpptools/count_kmer.cpp:139-170, and the per-occurrence table lookups of cpptools/count_kmer.cpp:86-96.
//
// Why: the key-partitioned pipeline of kernels.hip moves one 8-byte record per k-mer OCCURRENCE through two scatter
// passes and two LDS-table passes (20.8 GB per trip at 10 M read pairs).  Here a k-mer's bucket is a hash of its MINIMIZER
// (pg_device.hpp), consecutive k-mers of a read share it, and what travels is the SUPER-k-mer: one 12-byte record
//     bases : uint64  the 32 characters ending at the record's last character, stream order (oldest in the low bits)
//     meta  : uint32  row << 12 | (n - 1) << 8 | d2      row = index of the row the k-mers lie in (MINI_ROW_NONE: none),
//                                                        n = k-mers in the record (they end at the last n characters),
//                                                        d2 = the bucket's second-pass digit
// for a run of n <= 16 k-mers (about 4.3 on 150 bp reads, k = 21), i.e. under 3 bytes per occurrence.  The bucket
// workgroups re-derive the k-mers: forward codes are shifts of the character-reversed word, reverse-complement codes are
// shifts of the complemented word -- one reversal per record, two shifts and a compare per k-mer.
//
// Launches of one count (10 M pairs: 94 M words, ~600 M records):
//   mini_plan_kernel      (pg_mini_plan; depends on the stream, the rows and the geometry only) records per bucket and,
//                         per 4096-word chunk, records per first-pass region  -> scans -> exact offsets
//   mini_scatter_kernel   A1': one 512-thread workgroup per chunk, 512 words per round; a lane segments its word, ranks its
//                         records with one LDS atomic each, the round is laid out region-sorted in LDS and copied out
//   mini_scatter2_kernel  A2': every region -> its buckets (LDS multisplit, one global cursor add per digit and tile)
//   mini_count_kernel     B' + S1': one workgroup per bucket, 8-byte LDS slots (canonical code << 22 | count); the packed
//                         slice is written once; then the counts become bins in place and the records are read again
//                         (L2 / MALL) and looked up: (row, bin) words for the row shuffle of kernels.hip
#include <type_traits>

#include "pg_device.hpp"

namespace {

constexpr int S1_BLOCK = 512;                          // threads of a first-pass workgroup (256 VGPRs per lane: no spills)
constexpr int ROUND_WORDS = S1_BLOCK;                  // words per round of the first pass: one per lane
constexpr int MINI_CHUNK_WORDS = 4096;                 // words per chunk (one workgroup of the first pass)
constexpr int ROUNDS_PER_CHUNK = MINI_CHUNK_WORDS / ROUND_WORDS;
constexpr int STAGE_CAP = 8 * S1_BLOCK;                // records of a (sub-)round staged in LDS: 8 positions x 512 lanes always fit
constexpr int META_D2_BITS = 8, META_LEN_BITS = 4, META_ROW_SHIFT = META_D2_BITS + META_LEN_BITS;
constexpr uint32_t MINI_ROW_NONE = (1u << (32 - META_ROW_SHIFT)) - 1u;
// MASKED forms (pg_mini_plan_masked / pg_mini_count_half_masked): a record whose k-mers are valid for the rows but not for the table
// (bases below the quality threshold) carries this bit on top of its row -- rows stay below PG_MINI_MASKED_MAX_ROWS + 1 there, so a
// flagged row is never MINI_ROW_NONE -- and the count half adds nothing for it (the bit is cleared in the meta plane it leaves)
constexpr uint32_t MINI_ROW_NOTAB = 1u << (31 - META_ROW_SHIFT);
static_assert(PG_MINI_MASKED_MAX_ROWS < (int)MINI_ROW_NOTAB - 1, "a flagged row is never MINI_ROW_NONE");
constexpr int MINI_MAX_LEN = 1 << META_LEN_BITS;       // k-mers per record
constexpr int MINI_BITS1 = 8;                          // first-pass digits (regions); a table of 2^16 buckets: 2^8 regions x 2^8 buckets each
constexpr int MINI_MAX_BITS1 = 8;
#ifndef PG_SHORT_MAX
#define PG_SHORT_MAX 4
#endif
constexpr int PG_SHORT_MAX_ = PG_SHORT_MAX;                       // a record with at most this many k-mers is "short" (see mini_count_kernel)
static_assert(PG_MINI_MAX_ROWS == (int)MINI_ROW_NONE - 1, "row field of the record");
static_assert(PG_MINI_MAX_LOG2_BUCKETS == MINI_MAX_BITS1 + META_D2_BITS, "bucket id = region digit + second-pass digit");

struct MiniView {
    uint64_t *slots;
    int log2_slots, log2_bucket, k;
    __device__ __forceinline__ int bits() const { return log2_slots - log2_bucket; }
};

// first row whose end lies beyond the first character of each round (rows sorted, disjoint)
__global__ __launch_bounds__(BLOCK) void round_rows_kernel(const int64_t *__restrict__ row_end, int64_t n_rows, int64_t word_begin,
                                                           int64_t n_rounds, int32_t *__restrict__ round_row)
{
    const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_rounds) return;
    const int64_t c0 = (word_begin + t * ROUND_WORDS) * 32;
    int64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (row_end[mid] > c0) hi = mid; else lo = mid + 1;
    }
    round_row[t] = (int32_t)lo;
}

// ---- segmentation of ONE word into super-k-mer records.  A record is a maximal run of consecutive valid k-mers of the word
// (records never cross words: the lane that owns the word sees the k - 1 characters before it, like every stream reader
// here) that share their bucket and their row, capped at `cap` k-mers.  emit(e, n, bucket, row) is called once per record, e =
// position of its last character in the word; e is a compile-time constant at every call site (the position loop is fully
// unrolled), so callers may index register arrays with it.  The plan kernel and the scatter kernel both call this: they
// see the same records by construction.
struct RowBits {
    // where the rows (sorted, disjoint character ranges) cut the lane's 32 characters: bit p of `starts` = a row starts at
    // character p (p > 0), bit p of `ends` = character p is the first one behind a row; r0 = the row that holds character 0
    // (inside0) or the next row to start.  No per-position loop is needed afterwards.
    uint32_t starts, ends, r0;
    bool inside0;
    __device__ __forceinline__ void init(const int64_t *__restrict__ row_start, const int64_t *__restrict__ row_end, int64_t n_rows, int64_t first, int64_t pos0)
    {
        starts = ends = 0; r0 = 0; inside0 = false;
        if (!row_start) return;
        int64_t r = first;
        while (r < n_rows && row_end[r] <= pos0) ++r;           // first row that ends behind character 0
        r0 = (uint32_t)r;
        inside0 = r < n_rows && row_start[r] <= pos0;
        for (; r < n_rows; ++r) {
            const int64_t a = row_start[r] - pos0, b = row_end[r] - pos0;
            if (a >= 32) break;
            if (a > 0) starts |= 1u << a;
            if (b < 32) ends |= 1u << b;
        }
    }
    __device__ __forceinline__ uint32_t cuts() const { return starts | ends; }
    // bit p: character p lies inside a row (at(p) != MINI_ROW_NONE) -- a prefix XOR of the positions where that changes
    __device__ __forceinline__ uint32_t inside() const
    {
        uint32_t x = starts ^ ends;                             // (a row that ends where the next one starts changes nothing)
        x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
        return inside0 ? ~x : x;
    }
    // row of character p, MINI_ROW_NONE outside every row
    __device__ __forceinline__ uint32_t at(int p) const
    {
        const uint32_t upto = p == 31 ? 0xffffffffu : (2u << p) - 1u;
        const int s = __popc(starts & upto), e = __popc(ends & upto);
        const int inside = (inside0 ? 1 : 0) + s - e;
        return inside > 0 ? r0 + (uint32_t)s - (inside0 ? 0u : 1u) : MINI_ROW_NONE;
    }
};

// The segmentation in two steps that the plan kernel and the scatter kernel share (they see the same records by construction):
//   mini_minimizers   per_pos(p, mv) for p = 0 .. 31 (p a compile-time constant at every call): mv = the minimizer value of the
//                     k-mer that ends at character p of the word;
//   mini_record_ends  from the lane's validity masks and the mask of positions whose minimizer value equals their predecessor's:
//                     the positions where a record ENDS.  Pure bit arithmetic on 32-bit masks: until round 4 the record logic
//                     ran position by position (a counter, four comparisons, a predicated block per position that the whole
//                     wavefront issued although a word has six or seven records).
// A record's bucket is mini_bucket(mv of its last k-mer) -- all its k-mers share the value --, its length and row follow from where
// it ends (the callers keep the bucket of EVERY position in an LDS column of the lane and walk over the set bits of the end mask).
// DELAY (k > 21): the minimizer of a k-mer is taken over its central W M-mers only (pg_device.hpp: mini_window), i.e. the
// window that ends `off` characters before the k-mer does -- the window minimum passes through a delay line of `off` <= 5 steps.
// The forms themselves -- the canonical M-mer in six instructions, the window minimum in two, the "same value as before" mask in
// two -- are in mini_forms.hpp, where host code can compile and check them against the definition.
template <int W, bool DELAY, int M, class PerPos>
__device__ __forceinline__ void mini_minimizers(const Word &x, int off, PerPos &&per_pos)
{
    mini_minimizers_of_word<W, DELAY, M>(x.pw, x.cw, off, per_pos);
}

// bit p of the result: bits p - n + 1 .. p of m are all set (1 <= n <= 32)
__device__ __forceinline__ uint32_t runs32(uint32_t m, int n)
{
    uint32_t r = m;
    int len = 1;
    while (2 * len <= n) { r &= r << len; len *= 2; }
    if (len < n) r &= r << (n - len);
    return r;
}

// Where the records of a word end.  ok / ok_row: positions that end a valid k-mer (for the table / for the rows), cuts: positions
// where the row changes, eq: positions whose minimizer value equals that of the position before, cap: k-mers per record at most.
// A k-mer CONTINUES the open record if it and its predecessor are valid and of the same kind (row-counting or not), no row boundary
// lies at its last character and the minimizer value is the same (records never cross words: position 0 continues nothing) -- and
// if the record has room: of `cap` continuations in a row the last one starts a new record instead (lowest first, as a counter
// running over the positions would have it; rare -- a minimizer covers at most W = cap k-mers unless the same hashed M-mer recurs).
__device__ __forceinline__ uint32_t mini_record_ends(uint32_t ok, uint32_t ok_row, uint32_t cuts, uint32_t eq, int cap)
{
    uint32_t cont = ok & (ok << 1) & ~(ok_row ^ (ok_row << 1)) & ~cuts & eq;
    if (cap <= 1) cont = 0;
    else {
        uint32_t over = runs32(cont, cap);
        while (over) {                                          // (cont has a run of `cap` bits: the record would hold cap + 1 k-mers)
            cont &= ~(over & (0u - over));
            over = runs32(cont, cap);
        }
    }
    return ok & ~(cont >> 1);                                   // a record ends where the next position does not continue it
}

// what a lane needs to segment word w: the word, its valid k-mer ends under the counting rule and under the rows' strict rule
struct LaneWord {
    Word x;
    uint32_t ok, ok_row;
};
__device__ __forceinline__ LaneWord load_lane_word(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                   const uint32_t *__restrict__ strict, int64_t w, int k)
{
    LaneWord lw;
    lw.x = load_word(codes, valid, w, k);
    lw.ok = lw.x.ok;
    lw.ok_row = lw.ok;
    if (strict && lw.ok) {
        const uint32_t sv = strict[w], sp = w > 0 ? strict[w - 1] : 0u;
        lw.ok_row &= (uint32_t)(runs_of(((uint64_t)sv << 32) | sp, k) >> 32);
    }
    return lw;
}

// MASKED (the segmented plane `valid` is U = table plane | strict plane): a lane's k-mer ends of U split by the two rules.  T: valid
// under the table plane (counts in the table); R: valid under the strict plane (ok_row, belongs to the row it lies in).  A k-mer is
// kept if T holds, or if R holds inside a row (a row-only k-mer is looked up, not counted); one that mixes a base only the table
// takes with a base only the rows take is neither.  Records are also cut where T changes, so a record is all T or all not-T.
// Returns the lane's T ends; lw.ok becomes the kept ends, cuts gains the T changes.
__device__ __forceinline__ uint32_t mask_lane_word(LaneWord &lw, const RowBits &rb, uint32_t &cuts, const uint32_t *__restrict__ tabv, int64_t w, int k)
{
    const uint32_t tv = tabv[w], tp = w > 0 ? tabv[w - 1] : 0u;
    const uint32_t ok_tab = lw.ok & (uint32_t)(runs_of(((uint64_t)tv << 32) | tp, k) >> 32);
    lw.ok = ok_tab | (lw.ok_row & rb.inside());
    cuts |= ok_tab ^ (ok_tab << 1);
    return ok_tab;
}

// ---- plan: per chunk, records per first-pass region (chunk_hist[d * n_chunks + slot(chunk)]).  Nothing else: the per-bucket
// counts are taken from the records themselves once the first pass has written them (mini_bucket_hist_kernel).  With 2 KB of
// LDS, 256 threads and ~48 registers this kernel fits beside the workgroups of the other kernels on a CU -- beside the count
// kernel, which fills LDS but leaves half of the VALU issue slots and a third of the registers idle: KmerTable.prefetch_plan
// runs the next batch's plan on a side stream UNDER this batch's second scatter pass and count instead of in front of them
template <int W, bool DELAY, int M, bool MASKED = false>
__global__ __launch_bounds__(BLOCK) void mini_plan_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                          int64_t word_begin, int64_t word_end, int k, int woff, int bits, int bits2, int cap,
                                                          const int64_t *__restrict__ row_start, const int64_t *__restrict__ row_end, int64_t n_rows,
                                                          const uint32_t *__restrict__ strict, const int32_t *__restrict__ round_row,
                                                          unsigned long long *__restrict__ chunk_hist, int64_t n_chunks, int64_t chunk_stride,
                                                          unsigned long long *__restrict__ class_totals, const uint32_t *__restrict__ tabv)
{
    __shared__ uint32_t coarse[1 << MINI_MAX_BITS1];
    __shared__ uint32_t n_long_here;                             // records of more than SHORT_MAX k-mers in this chunk
    __shared__ uint32_t col[8 * BLOCK];                          // the region byte of every position of the lane's word (a column per lane,
                                                                 // four positions to a dword: region_bytes_push)
    const int bits1 = bits - bits2, n_dig = 1 << bits1;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        for (int i = threadIdx.x; i < (1 << MINI_MAX_BITS1); i += BLOCK) coarse[i] = 0;
        if (threadIdx.x == 0) n_long_here = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < MINI_CHUNK_WORDS; i += BLOCK) {
            const int64_t wi = chunk * MINI_CHUNK_WORDS + i;        // word index inside the range
            const int64_t w = word_begin + wi;
            if (w >= word_end) continue;
            LaneWord lw = load_lane_word(codes, valid, strict, w, k);
            if (lw.ok == 0) continue;
            RowBits rb;
            rb.init(row_start, row_end, n_rows, row_start ? round_row[wi / ROUND_WORDS] : 0, w << 5);
            uint32_t cuts = rb.cuts();
            if constexpr (MASKED) mask_lane_word(lw, rb, cuts, tabv, w, k);
            uint32_t eq = 0, prev = 0, acc = 0;
            mini_minimizers<W, DELAY, M>(lw.x, woff, [&](int p, uint32_t mv) {
                if (p > 0) eq_mask_push(eq, mv, prev);
                prev = mv;
                acc = region_bytes_push(acc, mv);
                if ((p & 3) == 3) col[(p >> 2) * BLOCK + threadIdx.x] = acc;
            });
            const uint32_t has = mini_record_ends(lw.ok, lw.ok_row, cuts, eq_mask_finish(eq), cap);
            // (the column is the lane's own: no barrier between its writes and these reads)
            for (uint32_t m = has; m; m &= m - 1u) {
                const int e = __builtin_ctz(m);
                atomicAdd(&coarse[region_of_bytes(col[(e >> 2) * BLOCK + threadIdx.x], e, bits1)], 1u);
            }
            // records of more than SHORT_MAX k-mers: ends with SHORT_MAX positions in front of them that neither end a record nor
            // fail to end a k-mer
            const uint32_t nonk = has | ~lw.ok;
            uint32_t lg = has & ~((1u << PG_SHORT_MAX_) - 1u);
#pragma unroll
            for (int q = 1; q <= PG_SHORT_MAX_; ++q) lg &= ~(nonk << q);
            if (lg) atomicAdd(&n_long_here, (uint32_t)__popc(lg));
        }
        __syncthreads();
        if (threadIdx.x == 0 && n_long_here) atomicAdd(class_totals, (unsigned long long)n_long_here);     // header[2]: long records of the stream
        for (int d = threadIdx.x; d < n_dig; d += BLOCK)
            chunk_hist[(int64_t)d * n_chunks + (int64_t)(((__int128)chunk * chunk_stride) % n_chunks)] = coarse[d];
        __syncthreads();
    }
}

// row sums of table[d][0..n): one workgroup per digit
__global__ __launch_bounds__(BIG_BLOCK) void digit_totals_kernel(const unsigned long long *__restrict__ table, int64_t n,
                                                                 unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long part[BIG_BLOCK / 64];
    const unsigned long long *row = table + (int64_t)blockIdx.x * n;
    unsigned long long s = 0;
    for (int64_t i = threadIdx.x; i < n; i += BIG_BLOCK) s += row[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < BIG_BLOCK / 64; ++i) run += part[i];
        totals[blockIdx.x] = run;
    }
}

// records per bucket, from the records the first pass has written: region = blockIdx.x / tiles_x holds [region_off[region],
// region_off[region + 1]); its workgroups count the second-pass digits of their share of the meta plane and add them to hist
__global__ __launch_bounds__(BLOCK) void mini_bucket_hist_kernel(const uint32_t *__restrict__ meta, const unsigned long long *__restrict__ region_off,
                                                                 int bits2, int tiles_x, unsigned long long *__restrict__ hist,
                                                                 const unsigned long long *__restrict__ header, unsigned long long rec_cap, const uint32_t *status)
{
    __shared__ uint32_t cnt[1 << META_D2_BITS];
    if (header[0] > rec_cap || (*status & PG_STATUS_PLAN_MISMATCH)) return;      // (a plan of another stream: see mini_count_kernel)
    const int n_dig = 1 << bits2;
    const uint32_t dmask = (uint32_t)n_dig - 1u;
    const int64_t region = blockIdx.x / tiles_x;
    const int64_t r0 = (int64_t)region_off[region], r1 = (int64_t)region_off[region + 1];
    if ((int)threadIdx.x < n_dig) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int64_t i0 = r0 + (int64_t)(blockIdx.x % tiles_x) * (8 * BLOCK); i0 < r1; i0 += (int64_t)tiles_x * (8 * BLOCK)) {
        uint32_t m[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t i = i0 + j * BLOCK + threadIdx.x;
            m[j] = i < r1 ? meta[i] : 0xffffffffu;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 + j * BLOCK + (int64_t)threadIdx.x < r1) atomicAdd(&cnt[m[j] & dmask], 1u);
    }
    __syncthreads();
    if ((int)threadIdx.x < n_dig && cnt[threadIdx.x]) atomicAdd(&hist[(region << bits2) + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// total records = off[nb] -> header[0]
__global__ void mini_total_kernel(const unsigned long long *__restrict__ off, int nb, unsigned long long *__restrict__ header)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) header[0] = off[nb];
}

// exclusive scan of cnt[0..N) -> start[0..N] by the first N / 64 wavefronts (N = 128 or 256); every lane of the workgroup calls
template <int N, bool LDS_ONLY = false>
__device__ __forceinline__ void scan_digits(const uint32_t *cnt, uint32_t *start, uint32_t *wave_tot, uint32_t *start_copy = nullptr)
{
    auto sync = [] { if (LDS_ONLY) lds_sync(); else __syncthreads(); };
    uint32_t v = 0, incl = 0;
    if (threadIdx.x < N) {
        v = cnt[threadIdx.x];
        incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d);
            if ((int)(threadIdx.x & 63) >= d) incl += o;
        }
        if ((threadIdx.x & 63) == 63) wave_tot[threadIdx.x >> 6] = incl;
    }
    sync();
    if (threadIdx.x < N) {
        uint32_t before = 0;
        for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) before += wave_tot[wv];
        start[threadIdx.x] = before + incl - v;
        if (start_copy) start_copy[threadIdx.x] = before + incl - v;
        if (threadIdx.x == N - 1) start[N] = before + incl;
    }
    sync();
}

// the same for N digits on BLK <= N threads: thread t owns the digits [t * N / BLK, (t + 1) * N / BLK)
template <int N, int BLK, bool LDS_ONLY = false>
__device__ __forceinline__ void scan_digits_blk(const uint32_t *cnt, uint32_t *start, uint32_t *wave_tot)
{
    constexpr int PER = N / BLK;
    static_assert(PER >= 1 && PER * BLK == N, "whole digits per thread");
    auto sync = [] { if (LDS_ONLY) lds_sync(); else __syncthreads(); };
    uint32_t v[PER], sum = 0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { v[q] = cnt[threadIdx.x * PER + q]; sum += v[q]; }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if ((int)(threadIdx.x & 63) >= d) incl += o;
    }
    if ((threadIdx.x & 63) == 63) wave_tot[threadIdx.x >> 6] = incl;
    sync();
    uint32_t base = incl - sum;
    for (int wv = 0; wv < (int)(threadIdx.x >> 6); ++wv) base += wave_tot[wv];
#pragma unroll
    for (int q = 0; q < PER; ++q) { start[threadIdx.x * PER + q] = base; base += v[q]; }
    if (threadIdx.x == BLK - 1) start[N] = base;
    sync();
}

// ---- A1': stream -> regions
// What a round stages in LDS is not the records but a 4-byte REFERENCE per record, region-sorted -- which lane's word it was cut
// from, where it ends, its bucket -- next to the lanes' words and masks; the record itself (32 characters, length, row) is put
// together by the copy-out thread that stores it.  The lane that segmented the word would have to do that in 32 predicated
// blocks, one per position a record may end at, every one of them issued for the whole wavefront although a word has six or
// seven records: the assembly cost 32 x ~30 vector instructions per word, in the copy-out it costs ~40 per RECORD at full lane
// occupancy (the first pass: 6.9 -> see DESIGN.md), and the stage shrinks from 13 to 4 bytes per record.
constexpr int REF_E_SHIFT = 16, REF_LANE_SHIFT = 21;               // ref = lane << 21 | e << 16 | bucket
static_assert(PG_MINI_MAX_LOG2_BUCKETS <= REF_E_SHIFT && S1_BLOCK <= (1 << (32 - REF_LANE_SHIFT)), "fields of a stage reference");
template <int N1> struct Scatter1Lds {                              // N1 regions: 256 (until round 4 also 512, for tables of 2^16 buckets: see Scatter2Lds)
    uint32_t ref[STAGE_CAP];
    uint16_t col[32 * S1_BLOCK];                                    // the bucket of every position of the lanes' words (a column per lane)
    uint64_t cw[S1_BLOCK], pw[S1_BLOCK];                            // the lanes' words and the words before them
    uint32_t nonk[S1_BLOCK];                                        // positions that end a record or end no k-mer at all
    uint32_t ok_row[S1_BLOCK];                                      // k-mer ends that count for rows
    uint32_t starts[S1_BLOCK], ends[S1_BLOCK], r0[S1_BLOCK];        // RowBits of the lane (r0: bit 31 = inside0)
    uint32_t cnt[N1];
    uint32_t start[N1 + 1];
    uint32_t fill[N1];                                              // start[], counted up as the references are placed
    // (512 regions: the array would push the structure 40 bytes over half of the CU's 160 KiB -- one workgroup per CU instead of
    // two; there the copy-out derives the value from cur[] and start[])
    unsigned long long gbase[N1 > 256 ? 1 : N1];
    unsigned long long cur[N1];                                     // running write offsets of this chunk, per region
    uint32_t wave_tot[N1 / 64];
};

static_assert(2 * sizeof(Scatter1Lds<256>) <= 160 * 1024, "two first-pass workgroups share a CU's LDS");
template <int N1> struct Scatter1LdsMasked : Scatter1Lds<N1> {
    uint32_t ok_tab[S1_BLOCK];                                      // MASKED: k-mer ends that count in the table (the rest are row-only)
};
static_assert(2 * sizeof(Scatter1LdsMasked<256>) <= 160 * 1024, "two first-pass workgroups share a CU's LDS");

template <int W, bool DELAY, int M, int N1, bool MASKED = false>
__global__ __launch_bounds__(S1_BLOCK, 4) void mini_scatter_kernel(const uint64_t *__restrict__ codes, const uint32_t *__restrict__ valid,
                                                                 int64_t word_begin, int64_t word_end, int k, int woff, int bits, int bits2, int cap,
                                                                 const int64_t *__restrict__ row_start, const int64_t *__restrict__ row_end, int64_t n_rows,
                                                                 const uint32_t *__restrict__ strict, const int32_t *__restrict__ round_row,
                                                                 uint64_t *__restrict__ out_bases, uint32_t *__restrict__ out_meta,
                                                                 const unsigned long long *__restrict__ chunk_off, int64_t n_chunks, int64_t chunk_stride,
                                                                 const unsigned long long *__restrict__ header, const unsigned long long *__restrict__ region_off,
                                                                 unsigned long long rec_cap, uint32_t *status, const uint32_t *__restrict__ tabv)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    static_assert(N1 <= S1_BLOCK, "one lane per region");
    if (header[0] > rec_cap) {                                      // (a plan of another stream: see mini_count_kernel)
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, PG_STATUS_PLAN_MISMATCH);
        return;
    }
    using Lds = std::conditional_t<MASKED, Scatter1LdsMasked<N1>, Scatter1Lds<N1>>;
    Lds &L = *reinterpret_cast<Lds *>(lds_raw);
    const int n_dig = 1 << (bits - bits2);
    const uint32_t d2mask = (1u << bits2) - 1u;
    const int64_t chunk = blockIdx.x;
    const int64_t slot = (int64_t)(((__int128)chunk * chunk_stride) % n_chunks);
    if (threadIdx.x < N1) L.cur[threadIdx.x] = (int)threadIdx.x < n_dig ? chunk_off[(int64_t)threadIdx.x * n_chunks + slot] : 0ull;
    for (int rd = 0; rd < ROUNDS_PER_CHUNK; ++rd) {
        const int64_t round = chunk * ROUNDS_PER_CHUNK + rd;
        const int64_t w = word_begin + round * ROUND_WORDS + threadIdx.x;
        if (word_begin + round * ROUND_WORDS >= word_end) break;    // (uniform)
        if (threadIdx.x < N1) L.cnt[threadIdx.x] = 0;
        lds_sync();                                                 // (also: the previous round's copy-out has read the lanes' words)
        // The lane's word -> the bucket of every position (an LDS column of the lane's own) and the mask of the positions where a
        // record ends; then the records are COUNTED per region, one LDS add without return per set bit (nothing waits for it).
        uint32_t has = 0;
        LaneWord lw;
        lw.ok = 0; lw.ok_row = 0; lw.x.cw = lw.x.pw = 0;
        if (w < word_end) lw = load_lane_word(codes, valid, strict, w, k);
        RowBits rb;
        rb.starts = rb.ends = rb.r0 = 0; rb.inside0 = false;
        uint16_t *const mycol = L.col + threadIdx.x;
        uint32_t ok_tab = 0;
        if (lw.ok) {
            rb.init(row_start, row_end, n_rows, row_start ? round_row[round] : 0, w << 5);
            uint32_t cuts = rb.cuts();
            if constexpr (MASKED) ok_tab = mask_lane_word(lw, rb, cuts, tabv, w, k);
            uint32_t eq = 0, prev = 0;
            mini_minimizers<W, DELAY, M>(lw.x, woff, [&](int p, uint32_t mv) {
                if (p > 0) eq_mask_push(eq, mv, prev);
                prev = mv;
                mycol[p * S1_BLOCK] = (uint16_t)mini_bucket(mv, bits);
            });
            has = mini_record_ends(lw.ok, lw.ok_row, cuts, eq_mask_finish(eq), cap);
            for (uint32_t m = has; m; m &= m - 1u)
                __hip_atomic_fetch_add(&L.cnt[(uint32_t)mycol[(uint32_t)__builtin_ctz(m) * S1_BLOCK] >> bits2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        // what the copy-out needs of this lane's word: a record's length and row follow from where it ends -- it starts behind the
        // previous record's end or behind the last position that ends no valid k-mer, whichever is later; its k-mers share one
        // row (that of its last character)
        L.cw[threadIdx.x] = lw.x.cw;
        L.pw[threadIdx.x] = lw.x.pw;
        L.nonk[threadIdx.x] = has | ~lw.ok;
        L.ok_row[threadIdx.x] = lw.ok_row;
        if constexpr (MASKED) L.ok_tab[threadIdx.x] = ok_tab;
        L.starts[threadIdx.x] = rb.starts;
        L.ends[threadIdx.x] = rb.ends;
        L.r0[threadIdx.x] = rb.r0 | (rb.inside0 ? 0x80000000u : 0u);
        lds_sync();
        scan_digits<N1, true>(L.cnt, L.start, L.wave_tot, L.fill);
        const uint32_t total = L.start[N1];
        // a round has at most 32 x 512 records; 8 positions x 512 lanes always fit the stage.  Nearly every round fits whole.
        const int n_win = total <= (uint32_t)STAGE_CAP ? 1 : 4;
        for (int win = 0; win < n_win; ++win) {
            const uint32_t wmask = n_win == 1 ? 0xffffffffu : (0xffu << (8 * win));
            if (n_win > 1) {                                        // count again, this window's records only
                lds_sync();
                if (threadIdx.x < N1) L.cnt[threadIdx.x] = 0;
                lds_sync();
                for (uint32_t m = has & wmask; m; m &= m - 1u)
                    __hip_atomic_fetch_add(&L.cnt[(uint32_t)mycol[(uint32_t)__builtin_ctz(m) * S1_BLOCK] >> bits2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                lds_sync();
                scan_digits<N1, true>(L.cnt, L.start, L.wave_tot, L.fill);
            }
            // gbase[d] = (where the region's run goes) - (where it starts in the stage): the copy-out adds the stage position
            if (threadIdx.x < N1) {
                const uint32_t c = L.start[threadIdx.x + 1] - L.start[threadIdx.x];
                if constexpr (N1 <= 256) L.gbase[threadIdx.x] = L.cur[threadIdx.x] - L.start[threadIdx.x];
                L.cur[threadIdx.x] += c;                            // (= gbase + start[d + 1])
            }
            {
                // the lane's records, two per turn: their buckets out of the column, their places in the stage from the regions'
                // fill counters (a returning add each, both in flight together), the references written
                const uint32_t mine = (uint32_t)threadIdx.x << REF_LANE_SHIFT;
                uint32_t m = has & wmask;
                while (m) {
                    const uint32_t e0 = (uint32_t)__builtin_ctz(m);
                    m &= m - 1u;
                    const bool two = m != 0u;
                    const uint32_t e1 = two ? (uint32_t)__builtin_ctz(m) : e0;
                    m &= m - 1u;                                    // (0 stays 0)
                    const uint32_t b0 = mycol[e0 * S1_BLOCK], b1 = mycol[e1 * S1_BLOCK];
                    const uint32_t p0 = __hip_atomic_fetch_add(&L.fill[b0 >> bits2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const uint32_t p1 = __hip_atomic_fetch_add(&L.fill[b1 >> bits2], two ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    L.ref[p0] = mine | (e0 << REF_E_SHIFT) | b0;
                    if (two) L.ref[p1] = mine | (e1 << REF_E_SHIFT) | b1;
                }
            }
            lds_sync();
            const uint32_t tot = L.start[N1];
            // copy-out: thread i puts record i of the region-sorted round together and stores it, two records at a time (their LDS
            // reads in flight together)
            for (uint32_t i0 = 0; i0 < tot; i0 += 2 * S1_BLOCK) {
                uint32_t rf[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t i = i0 + u * S1_BLOCK + threadIdx.x;
                    rf[u] = L.ref[i < tot ? i : 0u];                 // (tot > 0 here: ref[0] is a record)
                }
                uint64_t cwv[2], pwv[2];
                uint32_t nonk[2], okr[2], st[2], en[2], r0v[2], okt[2];
                unsigned long long gb[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t ln = rf[u] >> REF_LANE_SHIFT;
                    cwv[u] = L.cw[ln]; pwv[u] = L.pw[ln];
                    nonk[u] = L.nonk[ln]; okr[u] = L.ok_row[ln];
                    st[u] = L.starts[ln]; en[u] = L.ends[ln]; r0v[u] = L.r0[ln];
                    if constexpr (MASKED) okt[u] = L.ok_tab[ln]; else okt[u] = 0u;
                    const uint32_t d = (rf[u] & 0xffffu) >> bits2;
                    if constexpr (N1 <= 256) gb[u] = L.gbase[d];
                    else gb[u] = L.cur[d] - L.start[d + 1];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t i = i0 + u * S1_BLOCK + threadIdx.x;
                    const uint32_t e = (rf[u] >> REF_E_SHIFT) & 31u, b = rf[u] & 0xffffu;
                    const uint32_t below = nonk[u] & ((1u << e) - 1u);                       // ends / non-k-mers before e
                    const uint32_t n = below ? e - (31u - (uint32_t)__clz((int)below)) : e + 1u;
                    uint32_t row = MINI_ROW_NONE;
                    if ((okr[u] >> e) & 1u) {                                                // (RowBits::at)
                        const uint32_t upto = e == 31u ? 0xffffffffu : (2u << e) - 1u;
                        const int sc = __popc(st[u] & upto), ec = __popc(en[u] & upto);
                        const int in0 = (int)(r0v[u] >> 31);
                        if (in0 + sc - ec > 0) row = (r0v[u] & 0x7fffffffu) + (uint32_t)sc - (in0 ? 0u : 1u);
                    }
                    // (a row-only record lies inside a row by construction: mask_lane_word)
                    if (MASKED && !((okt[u] >> e) & 1u)) row |= MINI_ROW_NOTAB;
                    // the 32 characters ending at position e of the word
                    const uint64_t rec = e == 31u ? cwv[u] : (cwv[u] << (2u * (31u - e))) | (pwv[u] >> (2u * (e + 1u)));
                    const unsigned long long g = gb[u] + i;
                    // (a record beyond the buffers is dropped: cannot happen with the plan of THIS stream -- the offsets are exact --,
                    // and the plan of another one is reported below)
                    if (i < tot && g < rec_cap) {
                        out_bases[g] = rec;
                        out_meta[g] = (row << META_ROW_SHIFT) | ((n - 1u) << META_D2_BITS) | (b & d2mask);
                    }
                }
            }
        }
    }
    // every region's run of this chunk must end where the plan put the next chunk's: a plan that was computed for other reads
    // (KmerTable ties its cached plans to the stream; this is the backstop) shows here, and the count is void
    if ((int)threadIdx.x < n_dig) {
        const unsigned long long planned = slot + 1 < n_chunks ? chunk_off[(int64_t)threadIdx.x * n_chunks + slot + 1] : region_off[threadIdx.x + 1];
        if (L.cur[threadIdx.x] != planned) atomicOr(status, PG_STATUS_PLAN_MISMATCH);
    }
}

// ---- A2': region -> buckets.  tiles_x workgroups per region (all of them on one XCD, see below), its records are
// [off[region << bits2], off[(region + 1) << bits2]);
// digit = the low bits2 bits of meta (+ DIG / 2 for a LONG record: more than short_max k-mers).  Inside its bucket's range
// [off[b], off[b + 1]) the short records fill from the front (cursor[b]) and the long ones from the back (cursor_l[b]): the
// bucket workgroups treat a record in as many unrolled steps as its class can have k-mers, so sorting the two classes apart
// saves them the steps that short records would leave idle.  cursor[b] is the number of short records afterwards.
// DIG digits: 2 classes x 128 buckets of a region (tables of up to 2^15 buckets), or x 256 (2^16 buckets).  A tile is BLK x RPL
// records staged in LDS (12 bytes each); what the pass costs beyond a device copy is the partial 128-byte lines at the ends of
// the runs a tile appends to its digits, so both forms keep 16 or more records per digit and tile: 256 x 16 records for 256
// digits, 512 x 24 for 512 (until round 5 4096 records there too: runs of eight, 3.75 against 2.77 ms).  The larger tile takes
// 154 KiB of the CU's 160 KiB of LDS, one workgroup per CU, so its workgroups walk several tiles each and load the next tile
// into registers before they store the current one (PREFETCH).
template <int DIG, int BLK, int RPL> struct S2Geom {
    static constexpr int TILE = BLK * RPL;
    // kwords rides in the high half of the rank counters when a tile's k-mers stay below 2^16, else it has counters of its own
    static constexpr bool PACK_KW = TILE * MINI_MAX_WINDOW < 65536;
};
template <int DIG, int BLK, int RPL> struct Scatter2Lds {
    uint64_t bases[S2Geom<DIG, BLK, RPL>::TILE];
    uint32_t meta[S2Geom<DIG, BLK, RPL>::TILE];
    uint32_t cnt[DIG];
    uint32_t kw[S2Geom<DIG, BLK, RPL>::PACK_KW ? 1 : DIG];
    uint32_t start[DIG + 1];
    unsigned long long gbase[DIG];
    uint32_t wave_tot[BLK / 64];
};
template <int DIG, int BLK, int RPL, bool PREFETCH>
__global__ __launch_bounds__(BLK) void mini_scatter2_kernel(const uint64_t *__restrict__ in_bases, const uint32_t *__restrict__ in_meta,
                                                            const unsigned long long *__restrict__ off, int bits2, int tiles_x, int short_max,
                                                            uint64_t *__restrict__ out_bases, uint32_t *__restrict__ out_meta,
                                                            unsigned long long *__restrict__ cursor, unsigned long long *__restrict__ cursor_l,
                                                            unsigned long long *__restrict__ kwords,
                                                            const unsigned long long *__restrict__ header, unsigned long long rec_cap, uint32_t *status)
{
    if (header[0] > rec_cap || (*status & PG_STATUS_PLAN_MISMATCH)) return;      // (a plan of another stream: see mini_count_kernel)
    constexpr int TILE = S2Geom<DIG, BLK, RPL>::TILE;
    constexpr bool PACK_KW = S2Geom<DIG, BLK, RPL>::PACK_KW;
    // kwords[b] += the k-mers of bucket b that lie inside a row (= the words its workgroup will emit)
    static_assert(TILE < 65536 && DIG <= 65536, "rank and digit share a 32-bit word");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    Scatter2Lds<DIG, BLK, RPL> &L = *reinterpret_cast<Scatter2Lds<DIG, BLK, RPL> *>(lds_raw);
    constexpr int DPT = DIG / BLK;                              // digits per lane: threadIdx.x * DPT + q
    static_assert(DPT >= 1 && DPT * BLK == DIG, "whole digits per lane");
    constexpr uint32_t CLS = DIG / 2;                           // the class bit of a digit
    const int n_dig = 1 << bits2;
    const uint32_t dmask = (uint32_t)n_dig - 1u;
    // Workgroups go to the eight XCDs round-robin by their index, and each XCD has its own L2.  All workgroups of a region are put
    // on ONE XCD (region = index mod 8 + ...): the runs that the tiles of a region append to a bucket lie next to each other, so
    // the partial lines at their ends are completed in that L2 instead of being written back twice, half-filled, by two of them
    // (second pass 4.38 -> 2.97 ms on one box; all its stores left out: 1.60 ms, stored in tile order instead: 2.60 ms).
    const bool by_xcd = gridDim.x / (unsigned)tiles_x >= 8u;        // (a power of two of regions)
    const int64_t region = by_xcd ? (int64_t)(blockIdx.x % 8u) + 8 * (int64_t)((blockIdx.x / 8u) / (unsigned)tiles_x) : (int64_t)(blockIdx.x / tiles_x);
    const int64_t b0 = region << bits2;
    const int64_t r0 = (int64_t)off[b0], r1 = (int64_t)off[b0 + n_dig];
    const int64_t n_tiles = (r1 - r0 + TILE - 1) / TILE;
    auto digit_of = [&](uint32_t m) -> uint32_t {
        const int n = (int)((m >> META_D2_BITS) & (MINI_MAX_LEN - 1)) + 1;
        return (m & dmask) | (n > short_max ? CLS : 0u);
    };
    uint64_t rb[RPL];
    uint32_t rm[RPL], dr[RPL];
    auto load_tile = [&](int64_t t0) {                          // all loads of the lane in flight together
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int64_t i = t0 + j * BLK + threadIdx.x;
            rb[j] = i < r1 ? in_bases[i] : 0ull;
            rm[j] = i < r1 ? in_meta[i] : 0u;
        }
    };
    int64_t tile = by_xcd ? (blockIdx.x / 8u) % (unsigned)tiles_x : blockIdx.x % tiles_x;
    if (PREFETCH && tile < n_tiles) load_tile(r0 + tile * TILE);
    for (; tile < n_tiles; tile += tiles_x) {
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            L.cnt[threadIdx.x * DPT + q] = 0;
            if constexpr (!PACK_KW) L.kw[threadIdx.x * DPT + q] = 0;
        }
        lds_sync();
        const int64_t t0 = r0 + tile * TILE;
        if (!PREFETCH) load_tile(t0);
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int64_t i = t0 + j * BLK + threadIdx.x;
            if (i < r1) {
                const uint32_t d = digit_of(rm[j]);
                // (kwords == NULL: the merged lookups do not need the tally)
                const uint32_t kw = kwords && (rm[j] >> META_ROW_SHIFT) != MINI_ROW_NONE ? ((rm[j] >> META_D2_BITS) & (MINI_MAX_LEN - 1)) + 1u : 0u;
                if constexpr (PACK_KW) {
                    dr[j] = (d << 16) | (atomicAdd(&L.cnt[d], 1u | (kw << 16)) & 0xffffu);
                } else {
                    dr[j] = (d << 16) | atomicAdd(&L.cnt[d], 1u);
                    if (kw) atomicAdd(&L.kw[d], kw);
                }
            }
        }
        lds_sync();
        uint32_t kw_mine[DPT];                                      // (this lane's digits; the scan reads the same entries next)
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            if constexpr (PACK_KW) { kw_mine[q] = L.cnt[threadIdx.x * DPT + q] >> 16; L.cnt[threadIdx.x * DPT + q] &= 0xffffu; }
            else kw_mine[q] = L.kw[threadIdx.x * DPT + q];
        }
        if constexpr (DPT == 1) scan_digits<DIG, true>(L.cnt, L.start, L.wave_tot);
        else { lds_sync(); scan_digits_blk<DIG, BLK, true>(L.cnt, L.start, L.wave_tot); }
        // the returning cursor adds (one per digit and tile) are issued first and consumed after the placement
        unsigned long long gpos[DPT];
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            const uint32_t d = threadIdx.x * DPT + q;
            const uint32_t c = L.start[d + 1] - L.start[d];
            gpos[q] = 0;
            if (kw_mine[q]) atomicAdd(&kwords[b0 + (d & (CLS - 1u))], (unsigned long long)kw_mine[q]);
            if (c) {
                const int64_t b = b0 + (d & (CLS - 1u));
                gpos[q] = d < CLS ? off[b] + atomicAdd(&cursor[b], (unsigned long long)c) - L.start[d]
                                  : off[b + 1] - (atomicAdd(&cursor_l[b], (unsigned long long)c) + c) - L.start[d];
            }
        }
#pragma unroll
        for (int j = 0; j < RPL; ++j) {
            const int64_t i = t0 + j * BLK + threadIdx.x;
            if (i < r1) {
                const uint32_t at = L.start[dr[j] >> 16] + (dr[j] & 0xffffu);
                L.bases[at] = rb[j];
                L.meta[at] = rm[j];
            }
        }
        // (the lane's records are in LDS: its registers take the next tile while the workgroup stores this one)
        if (PREFETCH && tile + tiles_x < n_tiles) load_tile(r0 + (tile + tiles_x) * TILE);
#pragma unroll
        for (int q = 0; q < DPT; ++q) L.gbase[threadIdx.x * DPT + q] = gpos[q];
        lds_sync();
        const uint32_t total = L.start[DIG];
        for (uint32_t i = threadIdx.x; i < total; i += BLK) {       // flat sweep: the digit is in the record
            const uint32_t m = L.meta[i];
            const unsigned long long g = L.gbase[digit_of(m)] + i;
            gstore(out_bases, g, rec_cap, L.bases[i], status);
            gstore(out_meta, g, rec_cap, m, status);
        }
        lds_sync();
    }
}

// ---- B' + S1': one workgroup per bucket
//
// Count pass.  A lane owns one record per batch and treats its (up to CAP) k-mers in straight-line, fully unrolled code: all
// codes, all home slots and all first LDS probes of the record are issued before any is resolved (CAP independent LDS reads in
// flight per lane; the slots beyond the record's length are predicated off).  What the first probe does not settle -- a k-mer
// seen for the first time, a collision -- goes onto a small per-wavefront ring in LDS and is worked off 64 at a time by the
// general probing loop, so that loop always runs with every lane busy.
// Lookups.  An occurrence that lies in a row needs the FINAL count of its k-mer, which exists only when the bucket has been
// counted.  SLOTS form (rows < 2^(32 - log2 bucket slots)): the count pass leaves a provisional word (row, slot index) per
// occurrence -- it knows the slot when the insert is done -- and once the counts have become bins in place, the provisional
// words are streamed back (they are fresh in L2 / MALL) and turned into (row, bin) words by ONE LDS read each: no second
// derivation of the k-mers, no second probing.  General form: the records are read and probed a second time.
constexpr uint32_t RING_NOPLACE = 0xffff0000u;              // (MERGE: a ring entry of a k-mer outside every row; places stay below it)
constexpr int RING = 128;                                    // entries per wavefront ring: < 64 waiting + <= 64 pushed per step
constexpr int COUNT_WAVES = BIG_BLOCK / 64;
constexpr uint32_t BIN_NONE = (uint32_t)HASH_CMASK;          // a slot's count field after the counts have become bins: bin + 1, or this

// a value that is the same in every lane (read from LDS, say), moved to scalar registers: addresses built from it are a scalar
// base + a 32-bit lane offset, comparisons with it are scalar operands -- as vector registers such bases were spilled and
// reloaded in front of every load of an unrolled group, each reload with a wait for ALL memory operations in flight
__device__ __forceinline__ uint32_t uniform32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
template <class T> __device__ __forceinline__ T *uniform_ptr(T *p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    return reinterpret_cast<T *>(((uint64_t)uniform32((uint32_t)(v >> 32)) << 32) | uniform32((uint32_t)v));
}
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// the general insert; returns the slot the k-mer lives in, or 0xffffffff when the bucket is full (inactive lanes: 0).
// Written as ONE wave-uniform loop with two short predicated regions per round (claim an empty slot / add to a match): the
// structurizer's rendering of the obvious per-lane loop with early returns spends several times as many scalar
// instructions on mask bookkeeping, and those -- not the LDS -- were the cost of this path.
// WIDE (k > 21): tab[] holds code + 1 (0 = empty) and the counts live in their own 32-bit plane cnts[].
template <bool WIDE>
__device__ __forceinline__ uint32_t mini_insert_slow(unsigned long long *tab, uint32_t *cnts, uint32_t smask, uint32_t limit, uint64_t code, bool act, uint32_t skip = 0u)
{
    // (skip = 1: the first probe has seen the home slot taken by ANOTHER key -- nothing ever leaves a slot, so the search starts
    // behind it: one dependent LDS round trip less for most of what comes off the ring)
    uint32_t s = (mini_slot_hash<WIDE>(code) + skip) & smask;
    uint32_t res = act ? 0xffffffffu : 0u;
    bool todo = act;
    const unsigned long long fresh = WIDE ? (unsigned long long)(code + 1ull) : (unsigned long long)((code << HASH_CBITS) | 1ull);
    // one slot of the chain: claim it if it is empty, count on it if it holds the key; true when the lane is settled
    auto visit = [&](uint32_t at, unsigned long long cur) {
        if (todo && cur == 0) cur = atomicCAS(&tab[at], 0ull, fresh);
        const bool claimed = todo && cur == 0;
        if (WIDE) {
            const bool match = todo && cur == fresh;
            if (claimed || match) { atomicAdd(&cnts[at], 1u); res = at; todo = false; }
        } else {
            const bool match = todo && cur != 0 && (cur >> HASH_CBITS) == code;
            // stop growing at SAT; the overshoot is bounded by the lanes in flight and clamped when the slice is packed
            if (match && (uint32_t)(cur & HASH_CMASK) < HASH_SAT) atomicAdd(reinterpret_cast<uint32_t *>(&tab[at]), 1u);   // (the count is in the low dword)
            if (claimed || match) { res = at; todo = false; }
        }
    };
    // TWO slots per turn, both reads in flight together: a turn is a dependent LDS round trip (two where a slot is claimed), and
    // the round lasts as long as its longest chain.  The second slot is only visited by lanes whose first one holds another key
    // (what was read from it may be stale by then: a claim goes through compare-and-swap, which answers with what is there).
    for (uint32_t i = 0; i < limit; i += 2) {
        if (!__any(todo)) break;
        const uint32_t s1 = (s + 1) & smask;
        const unsigned long long cur0 = tab[s], cur1 = tab[s1];  // (settled lanes read their last slots again: harmless)
        visit(s, cur0);
        visit(s1, cur1);
        s = todo ? (s + 2) & smask : s;
    }
    return res;
}

// the general lookup: count field of `code` (BIN_NONE if absent)
template <bool WIDE>
__device__ __forceinline__ uint32_t mini_lookup_slow(const unsigned long long *tab, const uint32_t *cnts, uint32_t smask, uint32_t limit, uint64_t code, bool act)
{
    uint32_t s = mini_slot_hash<WIDE>(code) & smask;
    uint32_t res = BIN_NONE;
    bool todo = act;
    for (uint32_t q = 0; q < limit; ++q) {
        if (!__any(todo)) break;
        const unsigned long long cur = tab[s];
        const bool match = todo && (WIDE ? cur == code + 1ull : cur != 0 && (cur >> HASH_CBITS) == code);
        if (match) res = WIDE ? cnts[s] : (uint32_t)(cur & HASH_CMASK);
        if (match || cur == 0) todo = false;
        s = todo ? (s + 1) & smask : s;
    }
    return res;
}

// where the SLOTS form scatters its (row, bin) words: straight into the row shuffle's group regions (pg_shuffle_ctx)
struct ShufArgs {
    const unsigned long long *goff;
    unsigned long long *gcur1;
    uint32_t *words_out;
    int gb1, gb2, dshift;
    int narrow;                                                  // one-pass shuffle: 2-byte words (row inside its group, bin)
    unsigned long long words_cap;                                // 4-byte elements of words_out (checked builds)
};
// LDS of that scatter (bytes from the start of the dynamic area; the table has become 2-byte bins by then)
template <int BLK, int DIG> struct LookupLds {                 // BLK threads: 1024, or 512 (buckets of at most 2^13 slots: two workgroups per CU);
    static constexpr uint32_t TILE = 16 * BLK;                  // DIG row-group digits: 1024, or 2048 (65 537 .. 131 072 rows in one pass).  Words per tile: 16 per lane
    static constexpr uint32_t BUF = BLK == 1024 ? 32 * 1024 : 16 * 1024;        // (the 2-byte bins of the table's slots lie in front)
    static constexpr uint32_t CNT = BUF + 4 * TILE, START = CNT + 4 * DIG, GBASE = START + 4 * (DIG + 8), WAVE = GBASE + 8 * DIG, END = WAVE + 64;
};
constexpr int SHORT_MAX = PG_SHORT_MAX;                                 // a record with at most this many k-mers is "short"

// ---- the word-wise lookups of the slot form: provisional (row, slot) words -> (row, bin) words, 16 per lane and tile, scattered
// by the first digit of their row group into the row shuffle's regions (an LDS multisplit per tile, one global cursor add per
// digit and tile).  Called by a whole workgroup of BLK threads once the bucket's 2-byte bins lie at the start of the dynamic LDS:
// by the counting kernel while the counts are still there, or by mini_lookup_half_kernel.
struct WordCtx {
    unsigned char *lds;
    uint32_t smask, np;
    int lb, vbits;
    ShufArgs sh;
    uint32_t *status;
    const uint32_t *prov_b;
    unsigned long long *dbg;
};
template <int BLK, int DIG>
__device__ __forceinline__ void wordwise_lookup(const WordCtx &c)
{
    using FL = LookupLds<BLK, DIG>;
    constexpr int DPT = DIG / BLK;
    const uint16_t *bins16 = reinterpret_cast<const uint16_t *>(c.lds);
    uint32_t *buf = reinterpret_cast<uint32_t *>(c.lds + FL::BUF), *cnt = reinterpret_cast<uint32_t *>(c.lds + FL::CNT);
    uint32_t *start = reinterpret_cast<uint32_t *>(c.lds + FL::START), *wave_tot = reinterpret_cast<uint32_t *>(c.lds + FL::WAVE);
    unsigned long long *gbase = reinterpret_cast<unsigned long long *>(c.lds + FL::GBASE);
    const ShufArgs &sh = c.sh;
    const uint32_t smask = c.smask, np = c.np;
    const int lb = c.lb, vbits = c.vbits;
    uint32_t *const status = c.status;
    const uint32_t dmask = (1u << sh.gb1) - 1u;
#ifdef PG_MINI_STAMPS
    unsigned long long *dbg = c.dbg;
    unsigned long long tl = __builtin_amdgcn_s_memtime();
#define PG_LAP(K) do { if (threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); atomicAdd(&dbg[K], now_ - tl); tl = now_; } } while (0)
#else
#define PG_LAP(K) do { } while (0)
#endif
    // Software pipeline.  Every barrier in the loop is an LDS-only one (lds_sync), and there is ONE wait for global memory per
    // tile, in front of the copy-out: by then the next tile's words (requested at the top of the tile), the cursor adds
    // (requested as soon as the ranks, and with them the digits' counts, exist: in front of the scan) and the stores of the
    // previous tile's copy-out have had the whole tile to come back.  (vmcnt counts loads and stores in one queue: a wait
    // for the next words at the top of a tile would wait for the copy-out stores issued just before it.)
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t i = j * BLK + threadIdx.x;
        w[j] = i < np ? c.prov_b[i] : 0xffffffffu;
    }
    __builtin_amdgcn_s_waitcnt(0x0f70);                      // vmcnt(0): the first tile's words (no wait for w inside the loop)
    for (uint32_t t0 = 0; t0 < np; t0 += FL::TILE) {
#pragma unroll
        for (int q = 0; q < DPT; ++q) cnt[threadIdx.x * DPT + q] = 0;
        uint32_t wn[16];                                     // the next tile's words: in flight until the wait in front of the copy-out
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t i = t0 + FL::TILE + j * BLK + threadIdx.x;
            wn[j] = i < np ? c.prov_b[i] : 0xffffffffu;
        }
        lds_sync();                                          // (also: every wavefront is done with the previous tile's buffer)
        PG_LAP(16);
        // Every step below is written for all 16 words of the lane at once and without branches around the LDS operations -- 16
        // reads in flight and one wait, then 16 returning adds in flight and one wait (a word that is not placed adds 0 to some
        // counter): compiled from a per-word `if`, every word waited twice for a full LDS round trip
        uint32_t dr[16];
        uint32_t live = 0;
        {
            uint32_t b1[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) b1[j] = bins16[w[j] & smask];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t i = t0 + j * BLK + threadIdx.x;
                const bool ok = i < np && (uint32_t)(b1[j] - 1u) < 0xfffeu;        // a bin: not 0 (slot never filled), not 0xffff (out of range)
                w[j] = ((w[j] >> lb) << vbits) | (b1[j] - 1u);
                const uint32_t d = (w[j] >> sh.dshift) & dmask;
                dr[j] = (d << 16) | __hip_atomic_fetch_add(&cnt[d], ok ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                live |= ok ? 1u << j : 0u;
            }
        }
        lds_sync();
        PG_LAP(17);
        // this lane's digits: their words of the tile go to a range of the digit's region claimed with one global add
        unsigned long long g_region[DPT], g_claimed[DPT];
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            const uint32_t d = threadIdx.x * DPT + q, c_mine = cnt[d];
            g_region[q] = g_claimed[q] = 0;
            if (c_mine) {
                g_region[q] = sh.goff[(uint64_t)d << sh.gb2];
                g_claimed[q] = atomicAdd(&sh.gcur1[d], (unsigned long long)c_mine);
            }
        }
        scan_digits_blk<DIG, BLK, true>(cnt, start, wave_tot);
        PG_LAP(18);
        {
            uint32_t at[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) at[j] = start[dr[j] >> 16] + (dr[j] & 0xffffu);
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((live >> j) & 1u) buf[at[j]] = w[j];
        }
#pragma unroll
        for (int q = 0; q < DPT; ++q)                         // (the wait for global memory; unused for an empty digit)
            gbase[threadIdx.x * DPT + q] = g_region[q] + g_claimed[q] - start[threadIdx.x * DPT + q];
        lds_sync();
        PG_LAP(19);
        const uint32_t total = start[DIG];
        // copy-out, four words of the lane at a time (their LDS reads in flight together)
        for (uint32_t i0 = 0; i0 < total; i0 += 4 * BLK) {
            uint32_t r[4];
            unsigned long long g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = buf[i0 + u * BLK + threadIdx.x];            // (< FL::TILE: total <= FL::TILE = 16 blocks)
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = gbase[(r[u] >> sh.dshift) & dmask] + i0 + u * BLK + threadIdx.x;
            if (sh.narrow) {                                 // (the group region implies the rows' upper bits)
                uint16_t *out16 = reinterpret_cast<uint16_t *>(sh.words_out);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + u * BLK + threadIdx.x < total) gstore(out16, g[u], 2ull * sh.words_cap, r[u] & 0x7fffu, status);
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (i0 + u * BLK + threadIdx.x < total) gstore(sh.words_out, g[u], sh.words_cap, r[u], status);
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = wn[j];
        PG_LAP(20);
    }
}

// MERGE (SLOTS form only): the k-mers of a record share their row and, being neighbours in a read, mostly their bin.  The lookup
// phase then works record-wise: a lane takes ONE record of a batch, fetches the provisional words of its k-mers, turns them into
// bins and lets every run of equal neighbouring (row, bin) words travel on as ONE word with a count on top,
//     word = (run length - 1) << MERGE_CSHIFT | row << vbits | bin,
// so that ranks, region starts, staging and copy-out are paid per record and per run instead of per occurrence (measured on the
// bench workload: 0.28 words left per provisional word).
// The provisional data of this form lie in FIXED places, so that the lookup phase can fetch them without reading anything else
// first, and they are 2 bytes per k-mer: the bucket's range is
//     [ batches of short records: CXS rows of 64 halfwords each | batches of long records: CAP rows each ]
// and halfword (b x CX + j) x 64 + l of a class holds the SLOT of k-mer j of the record that lane l treated in batch b -- written
// exactly once: by the count loop when the first probe settled the k-mer, else by the general insert when it has found or made
// the slot (the ring carries the halfword's position next to the code).  Which halfwords mean anything follows from the record
// itself (its length and its row, re-read from the records' meta plane: batch b, lane l = record 64 b + l of its class), so
// nothing has to be cleared or marked, every occurrence of a record is in its lane's hands in the lookup phase (runs are never
// broken by k-mers that took the slow path) and the buffer's size follows from the classes' record counts alone, which the plan
// tallies (header[2]): 12 bytes per short record, 22 per long one, against 16 / 36 + a word per slow-path k-mer in round 3's first
// layout (4-byte (row, slot) words with 0xffffffff in the places of absent k-mers, the singles appended behind the batches).
constexpr int MERGE_CSHIFT = PG_SHUFFLE_COUNT_SHIFT;              // needs row bits + vbits <= 28 (mini_merge_form)
constexpr uint32_t WORD_NONE = 0xffffffffu;                       // (never a (row, bin) word: rows stay below 2^20 in this form)
struct MergeArgs {
    uint32_t *prov;                                              // the provisional slots of the MERGE form (halfwords, addressed as dwords)
    unsigned long long cap;                                      // its capacity, in dwords (the buckets claim their ranges on the word cursor)
};
// ---- the record-wise lookups of the MERGE form: provisional slots -> (run, row, bin) words, scattered by the first digit of
// their row group into the row shuffle's regions.  Called by a whole workgroup of BLK threads once the bucket's 2-byte bins lie
// at the start of the dynamic LDS (MergeLds layout).
struct MergeCtx {
    unsigned char *lds;                                          // dynamic LDS (bins16 first)
    uint32_t smask;
    int vbits;
    ShufArgs sh;
    uint32_t *status;
    const uint32_t *prov_b;                                      // the bucket's range (dwords of two slots)
    const uint32_t *meta_s, *meta_l;                             // meta words of the bucket's short / long records
    uint32_t n_s, n_l;                                           // ... and how many there are
    unsigned long long *dbg;                                     // PG_MINI_STAMPS builds: cycle sums of the phases (diagnostic)
};

// LDS of the MERGE form's lookup phase: the 2-byte bins in front, then the stage the wavefronts append their run words to --
// WPL words per lane, sorted IN PLACE: every lane keeps its WPL words and their places in registers across the scan (the first
// layouts of round 3 sorted into a second buffer of the same size instead, i.e. half the stage and twice the sort rounds per
// bucket: the kernel of those days had no registers to spare)
#ifndef PG_MERGE_WPL
#define PG_MERGE_WPL 24
#endif
template <int BLK, int DIG> struct MergeLds {
    static constexpr int WPL = (BLK == 1024 && DIG == 1024) ? PG_MERGE_WPL : (PG_MERGE_WPL < 20 ? PG_MERGE_WPL : 20);   // (144 KiB with 1024 threads, 72 KiB with 512: two workgroups per CU)
    static constexpr uint32_t TILE = WPL * BLK;                          // (>= 64 x 9 words per wavefront: what the wavefronts carry over from a full stage fits an empty one)
    static constexpr uint32_t BUF = BLK == 1024 ? 32 * 1024 : 16 * 1024;        // (the 2-byte bins of the table's slots lie in front)
    static constexpr uint32_t CNT = BUF + 4 * TILE, START = CNT + 4 * DIG, GBASE = START + 4 * (DIG + 8), WAVE = GBASE + 8 * DIG, END = WAVE + 64;
};
// a step of the lookup phase: two batches of short records or one batch of long ones per wavefront (a table whose records are
// not sorted into classes -- caps of at most PG_SHORT_MAX k-mers -- has short records only); KS k-mers per lane, NL loads per
// lane (the slot rows + the records' meta words)
template <int CAP> struct MergeStep {
    static constexpr bool TWO = CAP > PG_SHORT_MAX_;
    static constexpr int CXS = TWO ? PG_SHORT_MAX_ : CAP;
    static constexpr int KS = CAP > 2 * CXS ? CAP : 2 * CXS;
    static constexpr int NL = 2 + 2 * CXS;
    static constexpr int SLACK = 32 * (KS + 2);                                 // dwords a step may read behind the bucket's range (whole rows)
    static_assert(!TWO || (CAP <= 2 * CXS + 1 && NL == 10), "the long batch's rows fit the short step's loads");
};

template <int CAP, int BLK, int DIG>
__device__ __forceinline__ void merged_lookup(const MergeCtx &c)
{
    // Two stages, repeated until the bucket's records are used up (once or twice per bucket).
    // A (no barrier inside): every wavefront walks over its share of the work in STEPS -- two batches of short records (a lane
    //   takes one record of each) or one batch of long records --: fetch the slot rows and the records' meta words (one scalar base
    //   + constant offsets each, nothing to read first), turn the slots into bins, merge equal neighbouring (row, bin) words of a
    //   record into one word with a count, append the step's words to a stage of FL::TILE words in LDS (one returning add per
    //   step claims the positions).  The loads of the NEXT step are in flight meanwhile, and the wavefronts are at different
    //   points of the loop at any time.
    // B (when the stage is full or the work is done): the staged words are sorted by the first digit of their row group into a
    //   second buffer (WPL per lane: rank, scan, place) and copied out to the group regions, one global cursor add per digit.
    using FL = MergeLds<BLK, DIG>;
    using ST = MergeStep<CAP>;
    constexpr int DPT = DIG / BLK, WAVES_B = BLK / 64, WPL = FL::WPL;
    constexpr bool TWO = ST::TWO;
    constexpr int CXS = ST::CXS, KS = ST::KS, NL = ST::NL;
    constexpr uint32_t NONE = WORD_NONE;
    __shared__ uint32_t staged, valid_end, busy;
    const uint16_t *bins16 = reinterpret_cast<const uint16_t *>(c.lds);
    uint32_t *buf = reinterpret_cast<uint32_t *>(c.lds + FL::BUF), *cnt = reinterpret_cast<uint32_t *>(c.lds + FL::CNT);
    uint32_t *start = reinterpret_cast<uint32_t *>(c.lds + FL::START), *wave_tot = reinterpret_cast<uint32_t *>(c.lds + FL::WAVE);
    unsigned long long *gbase = reinterpret_cast<unsigned long long *>(c.lds + FL::GBASE);
    const ShufArgs &sh = c.sh;
    const int vbits = c.vbits;
    uint32_t *const status = c.status;
    const uint32_t *const prov_b = c.prov_b;
    // (one class only: its records -- handed over as the "long" ones, which is what the count loop's second range is -- are
    // treated two batches per step, as short records are)
    const uint32_t *const meta_s = TWO ? c.meta_s : c.meta_l, *const meta_l = c.meta_l;
    const uint32_t lane = lane_id(), wave = uniform32(threadIdx.x >> 6);
    const uint32_t half_lane = lane >> 1, parity_shift = (lane & 1u) * 16u;      // a row of 64 halfwords is read as 32 dwords: two lanes share one
    const uint32_t dmask = (1u << sh.gb1) - 1u;
    uint32_t *const wout = sh.words_out;
#ifdef PG_MINI_STAMPS
    unsigned long long tl_ = __builtin_amdgcn_s_memtime();
#define PG_MLAP(K) do { if (threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); atomicAdd(&c.dbg[48 + K], now_ - tl_); tl_ = now_; } } while (0)
#else
#define PG_MLAP(K) do { } while (0)
#endif
    const uint32_t n_s = uniform32(TWO ? c.n_s : c.n_l), n_l = TWO ? uniform32(c.n_l) : 0u;
    const uint32_t n_sb = (n_s + 63u) >> 6, n_lb = (n_l + 63u) >> 6;
    const uint32_t long_base = n_sb * 32u * CXS;                 // (dwords: a row of 64 slots is 32 of them)
    const uint32_t n_ss = (n_sb + 1u) >> 1;                      // steps of short batches, then one per long batch
    const uint32_t n_steps = n_ss + n_lb;
    if (n_steps == 0u) return;                                   // (uniform)
    // a step: first dword of its slot rows (A0), is it a step of short records (SHORT), first record of its (first) batch and the
    // records of its class (REC, NCLS)
    struct StepGeo { uint32_t a0, is_short, rec, ncls; };
    auto geometry = [&](uint32_t st) -> StepGeo {
        StepGeo g;
        if (!TWO || st < n_ss) { g.a0 = st * (64u * CXS); g.is_short = 1u; g.rec = st * 128u; g.ncls = n_s; }
        else { g.a0 = long_base + (st - n_ss) * (32u * CAP); g.is_short = 0u; g.rec = (st - n_ss) * 64u; g.ncls = n_l; }
        return g;
    };
    // the loads of a step: scalar bases and constant offsets (whole rows; what lies beyond the step's own rows is read and
    // ignored: the buffer has slack for it; a record index beyond its class is clamped).  Nothing is computed from the values here.
    //   w[0] = meta word of the lane's (first) record, w[1 + i] = slot row i, w[9] (two classes) = meta word of the second short
    //   record, or slot row 8 of a long one
    auto fetch_rows = [&](const StepGeo &g, uint32_t (&w)[NL]) {
        const uint32_t *rows = prov_b + g.a0;
        const uint32_t *meta_c = g.is_short ? meta_s : meta_l;
        const uint32_t last = g.ncls - 1u;
        const uint32_t ia = g.rec + lane < last ? g.rec + lane : last;
        w[0] = meta_c[ia];
#pragma unroll
        for (int i = 0; i < 2 * CXS; ++i) w[1 + i] = rows[32 * i + half_lane];
        {
            const uint32_t ib = g.rec + 64u + lane < last ? g.rec + 64u + lane : last;
            const uint32_t *p9 = g.is_short ? meta_c : rows + 32 * (2 * CXS);
            w[NL - 1] = p9[g.is_short ? ib : half_lane];
        }
    };
    // meta words + slots -> bins -> (row, bin) words; equal neighbours inside a record become ONE word with the run length on top
    auto process = [&](const StepGeo &g, const uint32_t (&r)[NL], uint32_t (&w)[KS]) {
        const uint32_t ma = r[0];
        const uint32_t row_a = ma >> META_ROW_SHIFT, n_a = ((ma >> META_D2_BITS) & (uint32_t)(MINI_MAX_LEN - 1)) + 1u;
        const bool ok_a = g.rec + lane < g.ncls && row_a != MINI_ROW_NONE;
        // the record that k-mer slots CXS .. KS - 1 belong to: the second short record, or the long one again
        uint32_t row_x = row_a, n_x = n_a;
        bool ok_x = ok_a;
        {
            const uint32_t mb = r[NL - 1];
            const uint32_t row_b = mb >> META_ROW_SHIFT, n_b = ((mb >> META_D2_BITS) & (uint32_t)(MINI_MAX_LEN - 1)) + 1u;
            const bool ok_b = g.rec + 64u + lane < g.ncls && row_b != MINI_ROW_NONE;
            row_x = g.is_short ? row_b : row_a;
            n_x = g.is_short ? n_b + (uint32_t)CXS : n_a;        // (a short record has at most CXS k-mers: slot 2 CXS is never its own)
            ok_x = g.is_short ? ok_b : ok_a;
        }
        uint32_t b1[KS];
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            // (no mask with the bucket's slot count: a halfword that means nothing may hold anything, and whatever it selects in
            // the 128 KiB behind the bins is read and ignored)
            const uint32_t pair = r[i < 2 * CXS ? 1 + i : NL - 1];
            b1[i] = bins16[__builtin_amdgcn_ubfe(pair, parity_shift, 16u)];
        }
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            const bool first = i < CXS;
            const bool ok = (first ? ok_a && (uint32_t)i < n_a : ok_x && (uint32_t)i < n_x) && b1[i] != 0xffffu;
            w[i] = ok ? ((first ? row_a : row_x) << vbits) | b1[i] : NONE;
        }
        // (from the last slot down: `run` = how many slots behind this one repeat it.  Two absent neighbours also count as "the same",
        // which never reaches a head: the run is reset where an absent slot follows a present one)
        uint32_t run = 0;
#pragma unroll
        for (int i = KS - 1; i >= 0; --i) {
            const uint32_t cur = w[i];
            const bool rec_start = i == 0 || (i == CXS && g.is_short);
            const bool same = !rec_start && cur == w[i > 0 ? i - 1 : 0];
            w[i] = same ? NONE : (run << MERGE_CSHIFT) | cur;     // (an absent slot stays absent: NONE is all ones)
            run = same ? run + 1u : 0u;
        }
    };
    // this thread's digits of a tile: claim their ranges in the group regions (one global add per digit and tile), scan
    auto claim_and_scan = [&]() {
        unsigned long long g_region[DPT], g_claimed[DPT];
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            const uint32_t d = threadIdx.x * DPT + q, c_mine = cnt[d];
            g_region[q] = g_claimed[q] = 0;
            if (c_mine) {
                g_region[q] = sh.goff[(uint64_t)d << sh.gb2];
                g_claimed[q] = atomicAdd(&sh.gcur1[d], (unsigned long long)c_mine);
            }
        }
        scan_digits_blk<DIG, BLK, true>(cnt, start, wave_tot);
#pragma unroll
        for (int q = 0; q < DPT; ++q)                             // (the wait for global memory; unused for an empty digit)
            gbase[threadIdx.x * DPT + q] = g_region[q] + g_claimed[q] - start[threadIdx.x * DPT + q];
    };
    if (threadIdx.x == 0) { staged = 0; valid_end = NONE; busy = 0; }
    uint32_t step = wave;                                        // this wavefront's next step
    bool pending = false;                                        // pw[] holds words that did not fit the stage yet (wave-uniform)
    uint32_t pw[KS];                                             // the words of the step in hand
    // the words of pw[] -> the stage; false (and nothing written) when they do not fit this round any more
    auto append = [&]() -> bool {
        // (the ballots are taken once and the lanes picked from the scalar masks: a predicate that crosses the branches below
        // would be re-materialised per use as v_cndmask + v_cmp)
        unsigned long long hm[KS];
        uint32_t n = 0;
#pragma unroll
        for (int j = 0; j < KS; ++j) { hm[j] = __builtin_amdgcn_ballot_w64(pw[j] != NONE); n += (uint32_t)__popcll(hm[j]); }
        if (n == 0) return true;                                 // (uniform)
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&staged, n);
        at = (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
        if (at + n > FL::TILE) {                                 // the stage is full: this step's words wait for the next round
            if (lane == 0) atomicMin(&valid_end, at);
            return false;
        }
#pragma unroll
        for (int j = 0; j < KS; ++j) {
            if (hm[j] == 0ull) continue;                         // (uniform)
            if (__builtin_amdgcn_inverse_ballot_w64(hm[j])) buf[at + lanes_below(hm[j])] = pw[j];
            at += (uint32_t)__popcll(hm[j]);
        }
        return true;
    };
    // one step: its loads are in `mine`; the next step's go out into `next` first, then the step is worked on and appended.
    // 0: done, 1: no step left, 2: the stage is full (the step's words stay in pw[])
    auto one_step = [&](uint32_t (&mine)[NL], uint32_t (&next)[NL]) -> int {
        if (step >= n_steps) return 1;                           // (uniform)
        const StepGeo g = geometry(step);
        step += WAVES_B;
        // (scheduling barriers: the compiler must neither sink these requests below the work on the step in hand nor pull
        // that work -- and with it the wait for what was just requested -- up in front of them)
        __builtin_amdgcn_sched_barrier(0);
        fetch_rows(geometry(step < n_steps ? step : 0u), next);  // the next step's loads: in flight while this one is worked on
        __builtin_amdgcn_sched_barrier(0);
        process(g, mine, pw);
        return append() ? 0 : 2;
    };
    lds_sync();
    for (;;) {
        // ---- A.  (What a full stage left in pw[] goes first: the stage is empty now.  The loads of `step` are requested again
        // behind every stage B, which had the registers; the two buffers swap roles from step to step: no copies)
        if (pending) pending = !append();                        // (a step's words always fit an empty stage: 64 KS words per wavefront)
        if (!pending) {
            uint32_t ca[NL], cb[NL];
            fetch_rows(geometry(step < n_steps ? step : 0u), ca);
            for (;;) {
                int r = one_step(ca, cb);
                if (r == 0) r = one_step(cb, ca);
                if (r) { pending = r == 2; break; }
            }
        }
        if (lane == 0 && (pending || step < n_steps)) atomicOr(&busy, 1u);
#pragma unroll
        for (int q = 0; q < DPT; ++q) cnt[threadIdx.x * DPT + q] = 0;     // (nobody reads the counters between the placement of one round and here)
        lds_sync();
        PG_MLAP(0);                                              // (stage A)
        const uint32_t n_valid = staged < valid_end ? staged : valid_end;
        const bool more = busy != 0u;
        // ---- B: the staged words [0, n_valid), WPL per lane (as many of them as the round has: uniform tests): rank, scan, place
        // -- in place: every word is in its lane's registers before the first barrier --, copy out
        {
            uint32_t w[WPL], at[WPL];
#pragma unroll
            for (int j = 0; j < WPL; ++j) w[j] = (uint32_t)(j * BLK) < n_valid ? buf[j * BLK + threadIdx.x] : 0u;
#pragma unroll
            for (int j = 0; j < WPL; ++j) {
                const uint32_t i = j * BLK + threadIdx.x;
                at[j] = 0;
                if ((uint32_t)(j * BLK) < n_valid)                  // (uniform)
                    at[j] = __hip_atomic_fetch_add(&cnt[(w[j] >> sh.dshift) & dmask], i < n_valid ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            lds_sync();
            if (threadIdx.x == 0) { staged = 0; valid_end = NONE; busy = 0; }     // (everybody has read them: a barrier lies in between)
            claim_and_scan();
#pragma unroll
            for (int j = 0; j < WPL; ++j)
                if ((uint32_t)(j * BLK) < n_valid) at[j] += start[(w[j] >> sh.dshift) & dmask];
#pragma unroll
            for (int j = 0; j < WPL; ++j)
                if ((uint32_t)(j * BLK) + threadIdx.x < n_valid) buf[at[j]] = w[j];
        }
        lds_sync();
        PG_MLAP(1);                                              // (ranks, cursor adds, scan, placement)
        // (not unrolled: the three iterations a full stage takes would each keep their own four 64-bit store bases -- wout + position
        // -- alive across the whole round loop: 24 vector registers, some of them spilled and reloaded in front of the stores with
        // a wait for every store in flight)
#pragma unroll 1
        for (uint32_t i0 = 0; i0 < n_valid; i0 += 4 * BLK) {
            uint32_t r[4];
            unsigned long long g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t i = i0 + u * BLK + threadIdx.x;
                r[u] = buf[i < FL::TILE ? i : 0u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] = gbase[(r[u] >> sh.dshift) & dmask] + i0 + u * BLK + threadIdx.x;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i0 + u * BLK + threadIdx.x < n_valid) gstore(wout, g[u], sh.words_cap, r[u], status);
        }
#ifdef PG_MINI_STAMPS
        if (threadIdx.x == 0) { atomicAdd(&c.dbg[48 + 6], 1ull); atomicAdd(&c.dbg[48 + 7], (unsigned long long)n_valid); }
#endif
        PG_MLAP(2);                                              // (copy-out)
        if (!more) break;                                        // (uniform)
        lds_sync();                                              // (the stage is free again: the next round's wavefronts may append)
    }
}

// HALF (N > 1 ranks; SLOTS form, packed slots): the COUNT half of the kernel.  The counts of a rank's own reads are not final --
// the other ranks hold occurrences of the same k-mers --, so instead of the slice and the lookups the bucket leaves
//   * its occupied slots (code << 22 | count) in slot order, compacted, in its slab of `ent` (the entries that travel to the
//     bucket's owner: pg_mini_gather_entries), their number in `fill`, and WHICH slots they are as a bitmap in `occ`;
//   * what the lookup half needs to find the bucket's provisional words (merged form: slots) again: where they start (`wbeg`)
//     (`ring_cnt`: the singles of the merged form's first layout; always 0 since the general insert writes into fixed places).
// mini_lookup_half_kernel finishes the bucket once the owner has answered with the bins of exactly these entries, in order.
// PIECES (one GPU, a stream counted in several word ranges because its scratch would not fit in one piece: pg_mini_count_piece):
// the same count half, but on the TABLE's own buckets -- the bucket's slice is loaded into LDS first (accum = 2; the first piece
// starts from an empty table: accum = 1), counted on, and written back; the slots keep their places from piece to piece (nothing
// ever leaves a slot), so the provisional slots of every piece stay valid until mini_lookup_slice_merge_kernel has looked them up
// in the final table.
// PIECES ON N > 1 RANKS (pg_mini_count_half_piece): the pieces count into the rank's LOCAL table as above (accum 1, 2), and the
// last one (accum 3; 4: a single piece, nothing to load) ends with the count half's epilogue instead of the write-back: entries,
// occupancy and fill are then exactly what one count half leaves, and mini_lookup_half_merge_kernel<..., PIECE> looks up every
// piece's provisional slots with the bins the owners sent back.
struct HalfArgs {
    unsigned long long *ent;                                     // bucket b: entries from b << log2 bucket slots
    unsigned long long *occ;                                     // bucket b: max(1, bucket slots / 64) words from b * that
    long long *fill;                                             // [buckets]
    uint32_t *ring_cnt;                                          // [buckets]
    int accum;                                                   // 0: N-rank count half; 1, 2: a piece; 3, 4: the last piece of a count half (see above)
    uint32_t *meta_w;                                            // MASKED: the meta plane the kernel reads, written back without MINI_ROW_NOTAB
};
// MASKED (pg_mini_count_half_masked; HALF and MERGE only): records flagged MINI_ROW_NOTAB take their slots as every record does
// but add 0 to the counts.  So that such a slot -- an all-A k-mer is code 0 -- never reads as empty, the count field of this form is
// biased by one (a claimed slot holds count + 1); the epilogues take the bias off, the entries then may have count 0.
template <int CAP, bool SLOTS, bool WIDE, int BLK, int DIG, bool MERGE = false, bool HALF = false, bool MASKED = false>
__global__ __launch_bounds__(BLK, 4) void mini_count_kernel(const uint64_t *__restrict__ bases, const uint32_t *__restrict__ meta,
                                                               const unsigned long long *__restrict__ off,
                                                               const unsigned long long *__restrict__ n_short,
                                                               const unsigned long long *__restrict__ kwords, MiniView t,
                                                               uint32_t window, uint32_t vsize, int vbits, uint32_t *__restrict__ words,
                                                               uint32_t *__restrict__ prov, unsigned long long *__restrict__ word_cursor,
                                                               unsigned long long *__restrict__ wbeg, unsigned long long *__restrict__ emit_end,
                                                               ShufArgs sh, MergeArgs mg, unsigned long long rec_cap, uint32_t *status, HalfArgs hv = HalfArgs{nullptr, nullptr, nullptr, nullptr, 0})
{
    static_assert(!MERGE || SLOTS, "merged words are a form of the slot lookups");
    static_assert(!HALF || (SLOTS && !WIDE), "the count half is a form of the slot lookups on packed slots");
    static_assert(!MASKED || (HALF && MERGE), "the masked form is a count half with the merged lookups");
#ifdef PG_MINI_GAPS                                              // (variant build for tools/wg_gaps.py: when a workgroup began and ended, and where)
    const unsigned long long gap_t0 = __builtin_amdgcn_s_memtime();
#endif
    // (the plan this launch was given describes another stream: its record count does not fit the record buffers -- nothing is
    // touched, bit 2 of the status word says so; KmerTable ties its cached plans to the stream, this is the backstop)
    if (word_cursor[-1] > rec_cap || (*status & PG_STATUS_PLAN_MISMATCH)) {     // (... or the first pass found the plan to be another stream's)
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, PG_STATUS_PLAN_MISMATCH);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ uint32_t emitted, emitted_ring;
    __shared__ unsigned long long n_lookups, wbase;
    __shared__ unsigned long long wave_words[(BLK / 64)];
    const uint32_t n_slots = 1u << t.log2_bucket;
    const uint32_t smask = n_slots - 1;
    const uint32_t limit = n_slots < MAX_PROBE ? n_slots : MAX_PROBE;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t *const cnts = reinterpret_cast<uint32_t *>(tab + n_slots);             // WIDE: the count plane behind the key plane
    const uint32_t tab_units = WIDE ? n_slots + n_slots / 2 : n_slots;              // 8-byte units of the table
    unsigned long long *ring = tab + tab_units + wave * RING;                        // [RING] codes of this wavefront
    uint32_t *ring_row = reinterpret_cast<uint32_t *>(tab + tab_units + (BLK / 64) * RING) + wave * RING;
    const int k = t.k, lb = t.log2_bucket;
    const uint64_t kmask = (1ull << (2 * k)) - 1ull;
    const int rc_sh0 = 2 * (32 - k);
    uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    uint32_t *slice_counts = reinterpret_cast<uint32_t *>(t.slots + (1ull << t.log2_slots)) + ((uint64_t)blockIdx.x << t.log2_bucket);   // WIDE
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    // [r0, rs) short records (at most SHORT_MAX k-mers; the second scatter pass put them first), [rs, r1) the others
    const int64_t rs = n_short && CAP > SHORT_MAX ? r0 + (int64_t)n_short[blockIdx.x] : r0;
    const bool emit_slots = SLOTS && window != 0;
    // every lane's first record of both classes, requested before anything else: with one workgroup per CU nothing hides a bucket's
    // start (bounds -> table cleared -> range claimed -> barrier -> first records -> first probes), so the records' round trip
    // runs under the clearing of the table and the claim
    const int64_t i_s = r0 + (int64_t)wave * 64 + lane, i_l = rs + (int64_t)wave * 64 + lane;
    const uint64_t first_s = i_s < rs ? bases[i_s] : 0ull, first_l = i_l < r1 ? bases[i_l] : 0ull;
    const uint32_t first_ms = i_s < rs ? meta[i_s] : 0xffffffffu, first_ml = i_l < r1 ? meta[i_l] : 0xffffffffu;
#ifdef PG_MINI_STAMPS
    unsigned long long *dbg = word_cursor + 7;                   // header[8..]: phase cycle sums (diagnostic build only)
    const unsigned long long st0 = __builtin_amdgcn_s_memtime();
#define PG_STAMP(K) do { __syncthreads(); if (threadIdx.x == 0) atomicAdd(&dbg[K], (unsigned long long)(__builtin_amdgcn_s_memtime() - st0)); } while (0)
    // per-wave laps inside the count loop: dbg[32 + K] += time since the previous lap (everything in flight is waited for first)
    unsigned long long wl = st0, wacc[5] = {0, 0, 0, 0, 0};
#if PG_MINI_STAMPS + 0 >= 2              // (-DPG_MINI_STAMPS=2: laps inside the count loop too -- every lap waits for all memory operations, which slows the loop down several times)
#define PG_WLAP(K) do { __builtin_amdgcn_s_waitcnt(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
                        wacc[K] += now_ - wl; wl = now_; } while (0)
#else
#define PG_WLAP(K) do { (void)wl; (void)wacc; } while (0)
#endif
#else
#define PG_STAMP(K) do { } while (0)
#define PG_WLAP(K) do { } while (0)
#endif
    if (HALF && (hv.accum == 2 || hv.accum == 3)) {              // (a later piece: the bucket as the pieces before left it)
        for (uint32_t i = threadIdx.x; i < tab_units; i += BLK) tab[i] = i < n_slots ? (unsigned long long)slice[i] : 0ull;
    } else {
        for (uint32_t i = threadIdx.x; i < tab_units; i += BLK) tab[i] = 0ull;
    }
    if (threadIdx.x == 0) { emitted = 0; emitted_ring = 0; n_lookups = 0; }
    if (emit_slots) {
        // every occurrence that lies in a row leaves exactly one word: the bucket's word range is claimed before the first word is
        // written (one global add).  The total comes with the records (the second scatter pass tallies it per bucket); without that
        // pass -- at most 256 buckets -- a pre-pass over the meta plane counts it.
        // (MERGE: nothing but fixed places, 2 bytes per k-mer of every batch of 64 records -- see MergeArgs; claimed in dwords)
        const unsigned long long fixed_words = MERGE ? 32ull * (unsigned long long)((rs - r0 + 63) >> 6) * (CAP > SHORT_MAX ? SHORT_MAX : CAP)
                                                       + 32ull * (unsigned long long)((r1 - rs + 63) >> 6) * CAP : 0ull;
        if (MERGE) {
            if (threadIdx.x == 0) wbase = atomicAdd(word_cursor, fixed_words);
        } else if (kwords) {
            if (threadIdx.x == 0) {
                n_lookups = kwords[blockIdx.x];
                wbase = atomicAdd(word_cursor, n_lookups);
            }
        } else {
            unsigned long long mine = 0;
            for (int64_t i0 = r0 + threadIdx.x; i0 < r1; i0 += BLK) {
                const uint32_t m = meta[i0];
                if ((m >> META_ROW_SHIFT) != MINI_ROW_NONE) mine += ((m >> META_D2_BITS) & (MINI_MAX_LEN - 1)) + 1;
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
            if (lane == 0) wave_words[wave] = mine;
            __syncthreads();
            if (threadIdx.x == 0) {
                unsigned long long run = 0;
                for (int w = 0; w < (BLK / 64); ++w) run += wave_words[w];
                n_lookups = run;
                wbase = atomicAdd(word_cursor, run);
            }
        }
    }
    __syncthreads();
    if (MERGE && emit_slots) {
        // (the word buffer was sized from the plan's record counts; a range that does not fit it -- a plan of other reads -- is
        // not written: bit 2 of the status word, as for the record buffers)
        const unsigned long long need = 32ull * (unsigned long long)((rs - r0 + 63) >> 6) * (CAP > SHORT_MAX ? SHORT_MAX : CAP)
                                        + 32ull * (unsigned long long)((r1 - rs + 63) >> 6) * CAP + (unsigned long long)MergeStep<CAP>::SLACK;
        if (wbase + need > mg.cap || 2ull * need >= (unsigned long long)RING_NOPLACE) {      // (uniform; places are 32-bit halfword numbers below RING_NOPLACE)
            if (threadIdx.x == 0) atomicOr(status, PG_STATUS_PLAN_MISMATCH);
            return;
        }
    }
    unsigned long long wb = emit_slots ? wbase : 0ull;
    // (read from LDS, hence a vector register to the compiler; made a scalar so that the words' addresses are a scalar base + a
    // 32-bit lane offset instead of a 64-bit sum per lane and load)
    wb = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(wb >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wb);
    uint32_t *const prov_b = (MERGE ? mg.prov : prov) + wb;      // the bucket's words (32-bit positions from here on)
    // words are placed by claiming positions on the bucket's LDS counter `emitted`: ONE returning add per batch of 64 records
    // (all its first-probe hits) and one per general insert round, by lane 0
    auto claim = [&](uint32_t n_words) -> uint32_t {
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&emitted, n_words);
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)at);
    };
    // MERGE: the bucket's range = batches of short records | batches of long records, a halfword per k-mer (see MergeArgs)
    constexpr uint32_t CXS_ = CAP > SHORT_MAX ? SHORT_MAX : CAP;
    const uint32_t n_sb = (uint32_t)((rs - r0 + 63) >> 6), n_lb = (uint32_t)((r1 - rs + 63) >> 6);
    const uint32_t long_base = n_sb * 64u * CXS_;                // (halfwords)
    const uint32_t np_half = long_base + n_lb * 64u * CAP;       // (... of the bucket, for the checked build)
    uint16_t *const prov_h = reinterpret_cast<uint16_t *>(prov_b);
    const uint32_t np_all = (uint32_t)n_lookups;                 // (emit_slots: the bucket's words, known before the first is written)
    PG_STAMP(0);
    bool full = false;
    unsigned long long mine = 0;                                 // k-mers of this lane's records that lie inside a row
    uint32_t head = 0, tail = 0;                                 // ring positions (wave-uniform)
    // one pending occurrence per lane off the ring: the general insert, and its word.
    // Packed slots (k <= 21): ONE turn per round.  A ring entry is code | next slot to visit << 42 | turns taken << 56; the round
    // reads that slot and the one behind it (both reads in flight), claims or counts, and a lane that is not settled by them puts
    // its entry BACK on the ring, two slots further on -- a round used to last as long as the longest probe chain among its 64
    // lanes (three to four dependent turns of three LDS round trips each, every other lane waiting), now a lane costs as many
    // turns as its own chain has (1.15 on average at load 0.35).  After 255 turns (510 slots) the bucket counts as full.
    constexpr uint64_t RING_CODE = (1ull << 42) - 1ull;
    constexpr int RING_SLOT_SHIFT = 42, RING_TURN_SHIFT = 56;
    static_assert(PG_BUCKET_MAX_LOG2_SLOTS <= RING_TURN_SHIFT - RING_SLOT_SHIFT, "a slot index fits its field of the ring entry");
    auto slow_round = [&](bool act) {
        const uint32_t at = (head + lane) & (RING - 1);
        const uint64_t c_ = act ? ring[at] : 0ull;
        constexpr uint32_t RING_NONE = MERGE ? 0xffffffffu : MINI_ROW_NONE;      // (MERGE: ring_row holds places, not rows; no place: anything from RING_NOPLACE on)
        const uint32_t rw = act && emit_slots ? ring_row[at] : RING_NONE;
        uint32_t sl;
        bool settled = act;                                      // (lanes whose word may be written this round)
        if constexpr (WIDE) {
            const uint64_t c = c_ & ~(1ull << 63);               // (bit 63: the home slot was taken by another key when the first probe looked)
            sl = mini_insert_slow<WIDE>(tab, cnts, smask, limit, c, act, (uint32_t)(c_ >> 63));
        } else {
            const uint64_t code = c_ & RING_CODE;
            const uint32_t s0 = (uint32_t)(c_ >> RING_SLOT_SHIFT) & smask, s1 = (s0 + 1u) & smask;
            // (MASKED: bit 63 = a row-only k-mer, the turns keep 7 bits)
            const uint32_t turns = MASKED ? (uint32_t)(c_ >> RING_TURN_SHIFT) & 0x7fu : (uint32_t)(c_ >> RING_TURN_SHIFT);
            const bool notab = MASKED && (c_ >> 63) != 0ull;
            const unsigned long long fresh = (unsigned long long)((code << HASH_CBITS) | (MASKED && !notab ? 2ull : 1ull));
            const unsigned long long cur0 = tab[s0], cur1 = tab[s1];
            bool todo = act;
            sl = act ? 0xffffffffu : 0u;
            // one slot of the chain: claim it if it is empty, count on it if it holds the key (what was read may be stale by now:
            // a claim goes through compare-and-swap, which answers with what is there)
            auto visit = [&](uint32_t slot, unsigned long long cur) {
                if (todo && cur == 0) cur = atomicCAS(&tab[slot], 0ull, fresh);
                const bool claimed = todo && cur == 0;
                const bool match = todo && cur != 0 && (cur >> HASH_CBITS) == code;
                // stop growing at SAT; the overshoot is bounded by the lanes in flight and clamped when the slice is packed
                const bool room = MASKED ? !notab && (uint32_t)(cur & HASH_CMASK) <= HASH_SAT : (uint32_t)(cur & HASH_CMASK) < HASH_SAT;
                if (match && room) atomicAdd(reinterpret_cast<uint32_t *>(&tab[slot]), 1u);   // (the count is in the low dword)
                if (claimed || match) { sl = slot; todo = false; }
            };
            visit(s0, cur0);
            visit(s1, cur1);
            // (a bucket with fewer slots than a lane may visit: it has seen them all)
            const bool give_up = todo && (turns == (MASKED ? 127u : 255u) || 2u * (turns + 1u) >= limit);
            const bool again = todo && !give_up;
            settled = act && !again;
            const unsigned long long am = __ballot(again);
            if (am) {                                            // (uniform; the round's own 64 places are free: they were read above)
                if (again) {
                    const uint32_t to = (tail + lanes_below(am)) & (RING - 1);
                    ring[to] = code | ((uint64_t)((s0 + 2u) & smask) << RING_SLOT_SHIFT) | ((uint64_t)(turns + 1u) << RING_TURN_SHIFT) | (notab ? 1ull << 63 : 0ull);
                    if (emit_slots) ring_row[to] = rw;
                }
                tail += (uint32_t)__popcll(am);
            }
        }
        full |= settled && sl == 0xffffffffu;
        if (emit_slots) {
            // (a full bucket still gets its word -- the slot of a k-mer that is not there reads as "no bin")
            const bool put = settled && (MERGE ? rw < RING_NOPLACE : rw != RING_NONE);
            const unsigned long long qm = __ballot(put);
            if (MERGE) {
                // (the ring carried the k-mer's own place among the bucket's halfwords instead of its row)
                if (put) gstore(prov_h, (uint64_t)rw, (uint64_t)np_half, (uint16_t)(sl == 0xffffffffu ? 0xffffu : sl & smask), status);
            } else
            if (qm) {                                            // (uniform)
                {
                    const uint32_t at = claim((uint32_t)__popcll(qm));
                    if (put) gstore(prov_b, (uint64_t)at + lanes_below(qm), (uint64_t)np_all, (rw << lb) | (sl & smask), status);
                }
            }
        }
    };
    // ---- count: wavefront w takes the batches [ra + 64 (w + 16 t), + 64) of a class; CX = k-mers per record at most there
    auto count_range = [&](auto cx, int64_t ra, int64_t rb, uint64_t R, uint32_t m) {       // (R, m: the lane's first record of the range, loaded at the top of the kernel)
        constexpr int CX = decltype(cx)::value;
        int64_t i = ra + (int64_t)wave * 64 + lane;
        for (int64_t i0 = ra + (int64_t)wave * 64; i0 < rb; i0 += BLK) {
            PG_WLAP(0);                                          // (loop top: the record has arrived, last batch's stores are out)
            const bool live = i0 + lane < rb;
            const int n = live ? (int)((m >> META_D2_BITS) & (MINI_MAX_LEN - 1)) + 1 : 0;
            uint32_t row = m >> META_ROW_SHIFT;
            bool notab = false;                                  // (MASKED) a row-only record: its k-mers add nothing
            if constexpr (MASKED) {
                notab = row != MINI_ROW_NONE && (row & MINI_ROW_NOTAB) != 0u;
                if (notab) {
                    row &= ~MINI_ROW_NOTAB;
                    gstore(hv.meta_w, (uint64_t)(i0 + lane), (uint64_t)rec_cap, m & ~(MINI_ROW_NOTAB << META_ROW_SHIFT), status);
                }
            }
            const bool in_row = live && row != MINI_ROW_NONE;
            // (MERGE) the lane's first halfword in the bucket's range: k-mer j of its record has place0 + 64 j
            const uint32_t place0 = (CX < CAP ? 0u : long_base) + (uint32_t)((i0 - ra) >> 6) * (64u * CX) + lane;
            // (what the ring carries for k-mer j is ring_place0 + 64 j: its place, or -- outside every row -- something at or beyond RING_NOPLACE)
            const uint32_t ring_place0 = row != MINI_ROW_NONE ? place0 : RING_NOPLACE;
            if (in_row) mine += (unsigned long long)n;
            const uint64_t FW = rev2_64(R), RC = R ^ 0xAAAAAAAAAAAAAAAAull;
            i = i0 + BLK + lane;                           // the next batch's loads fly during this one
            {
                // ... provided they are issued BEHIND the wait for this batch's record: the compiler hoists them to the top of the
                // loop, in front of that wait, and -- the loads being conditional -- the wait is an s_waitcnt vmcnt(0) that then
                // covers them too: every batch stood still for a full memory round trip (one workgroup per CU: nothing else to
                // run).  Making their address depend on this batch's record pins them behind the wait.
                const uint32_t arrived = (uint32_t)FW;
                asm volatile("" : "+v"(i) : "v"(arrived));
            }
            R = i < rb ? bases[i] : 0ull;
            m = i < rb ? meta[i] : 0xffffffffu;
            // Straight-line code from here to the ballots: the reads and the adds go out for every lane (a lane without a j-th k-mer
            // reads some slot and adds 0 to it), so that no predicate crosses a branch -- a predicate that does comes back as
            // v_cndmask + v_cmp per use, and the branches around each predicated add cost more than the add
            uint64_t code[CX];
            uint32_t sl[CX];
            unsigned long long cur[CX];
#pragma unroll
            for (int j = 0; j < CX; ++j) {                       // every first probe of the record in flight
                // k-mer j and its reverse complement, both pushed up to bit 63 (what lies below them is the same junk for the
                // comparison's purposes: the 2k bits on top decide, a palindrome gives the same code either way)
                const uint64_t fw = FW << ((rc_sh0 - 2 * j) & 63), rc = RC << (2 * j);        // (j beyond the cap: no such k-mer, any value will do)
                code[j] = (fw < rc ? fw : rc) >> rc_sh0;
                sl[j] = mini_slot_hash<WIDE>(code[j]) & smask;
                cur[j] = tab[sl[j]];
            }
            // (ballots of single comparisons, combined as scalars: the ballot of a compound predicate is compiled as
            // v_cndmask + v_cmp on top of the scalar logic)
            const unsigned long long in_row_m = __builtin_amdgcn_ballot_w64(row != MINI_ROW_NONE);
            const unsigned long long notab_m = MASKED ? __builtin_amdgcn_ballot_w64(notab) : 0ull;
            PG_WLAP(1);                                          // (codes, hashes, first probes back)
            unsigned long long pm[CX], qm[CX];                   // lanes whose j-th k-mer was settled by the first probe inside a row / is still pending
#pragma unroll
            for (int j = 0; j < CX; ++j) {
                const unsigned long long act = __builtin_amdgcn_ballot_w64(j < n);
                unsigned long long hit;
                if (WIDE) {
                    hit = act & __builtin_amdgcn_ballot_w64(cur[j] == code[j] + 1ull);
                    __hip_atomic_fetch_add(&cnts[sl[j]], __builtin_amdgcn_inverse_ballot_w64(hit) ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    hit = act & __builtin_amdgcn_ballot_w64(cur[j] != 0) & __builtin_amdgcn_ballot_w64((cur[j] >> HASH_CBITS) == code[j]);
                    // (the count sits in the low 22 bits of the slot's low dword and stops far below 2^22: a 32-bit LDS add is enough)
                    // (MASKED: the field holds count + 1 of an occupied slot; a row-only k-mer adds nothing)
                    const unsigned long long room = MASKED ? __builtin_amdgcn_ballot_w64((((uint32_t)cur[j] - 1u) & HASH_SAT) == 0) & ~notab_m
                                                           : __builtin_amdgcn_ballot_w64(((uint32_t)cur[j] & HASH_SAT) == 0);
                    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(&tab[sl[j]]), __builtin_amdgcn_inverse_ballot_w64(hit & room) ? 1u : 0u,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                pm[j] = hit & in_row_m;
                qm[j] = act & ~hit;
            }
            uint32_t at = 0;
            if (emit_slots) {
                // positions for the provisional words of the hits: the claim is issued here and used behind the ring pushes
                uint32_t total = 0;
#pragma unroll
                for (int j = 0; j < CX; ++j) total += (uint32_t)__popcll(pm[j]);
                if (total && !MERGE) at = claim(total);          // (uniform; the MERGE form's words have fixed places)
            }
            PG_WLAP(2);                                          // (hits added, positions claimed)
#pragma unroll
            for (int j = 0; j < CX; ++j) {
                const unsigned long long mask = qm[j];
                if (mask) {                                      // (uniform)
                    if (__builtin_amdgcn_inverse_ballot_w64(mask)) {
                        const uint32_t at = (tail + lanes_below(mask)) & (RING - 1);
                        // (a slot that is not empty and not a hit holds another key, and nothing ever leaves a slot: the search
                        // starts behind it)
                        if constexpr (WIDE) ring[at] = code[j] | (cur[j] != 0ull ? 1ull << 63 : 0ull);
                        else ring[at] = code[j] | ((uint64_t)((sl[j] + (cur[j] != 0ull ? 1u : 0u)) & smask) << RING_SLOT_SHIFT) | (notab ? 1ull << 63 : 0ull);
                        // (MERGE: the general insert writes the slot to the k-mer's own place: the ring carries that place)
                        if (emit_slots) ring_row[at] = MERGE ? ring_place0 + 64u * j : row;
                    }
                    tail += (uint32_t)__popcll(mask);
                    while (tail - head >= 64) {                  // (a round may put unsettled lanes back: at most as many as it took off)
#ifdef PG_MINI_STAMPS
                        const unsigned long long ts = __builtin_amdgcn_s_memtime();
#endif
                        slow_round(true);
                        head += 64;
#ifdef PG_MINI_STAMPS
                        if (lane == 0) atomicAdd(&dbg[6], (unsigned long long)(__builtin_amdgcn_s_memtime() - ts));     // per-wave time in the general insert
#endif
                    }
                }
            }
            PG_WLAP(3);                                          // (ring pushes, general inserts)
            if (emit_slots) {
                if (MERGE) {
                    // fixed places: halfword row j of the batch = the slots of the j-th k-mers of its 64 records; a k-mer that the
                    // first probe did not settle gets its slot from the general insert, one outside every row gets none
#pragma unroll
                    for (int j = 0; j < CX; ++j)
                        if (__builtin_amdgcn_inverse_ballot_w64(pm[j]))
                            gstore(prov_h, (uint64_t)place0 + 64u * j, (uint64_t)np_half, (uint16_t)sl[j], status);
                } else
                // the words, slot by slot (neighbours in the buffer come from different records: the row histograms behind the
                // shuffle do not like runs of equal words).  (Deferring these stores to the next iteration's top, behind its
                // vmcnt wait, changed nothing: 17.33 ms either way.)
                {
#pragma unroll
                for (int j = 0; j < CX; ++j) {
                    if (__builtin_amdgcn_inverse_ballot_w64(pm[j])) gstore(prov_b, (uint64_t)at + lanes_below(pm[j]), (uint64_t)np_all, (row << lb) | sl[j], status);
                    at += (uint32_t)__popcll(pm[j]);
                }
                }
            }
            PG_WLAP(4);                                          // (the words' stores, waited for)
        }
    };
    count_range(std::integral_constant<int, (CAP > SHORT_MAX ? SHORT_MAX : CAP)>{}, r0, rs, first_s, first_ms);
    count_range(std::integral_constant<int, CAP>{}, rs, r1, first_l, first_ml);
    while (tail != head) {                                       // what is left on the ring
        const uint32_t left = tail - head < 64u ? tail - head : 64u;
        slow_round(lane < left);
        head += left;
    }
#ifdef PG_MINI_STAMPS
    if (lane == 0) {
        atomicAdd(&dbg[5], (unsigned long long)(__builtin_amdgcn_s_memtime() - st0));     // per-wave end of the count loop
        for (int q = 0; q < 5; ++q) atomicAdd(&dbg[32 + q], wacc[q]);
    }
#endif
    PG_STAMP(1);
    if (full) atomicOr(status, 1u);
    if (window && !emit_slots) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
        if (lane == 0 && mine) atomicAdd(&n_lookups, mine);
    }
    __syncthreads();
    if (HALF && (hv.accum == 1 || hv.accum == 2)) {
        // a piece: the slice back (counts clamped: the adds stop at SAT, the overshoot of concurrent ones is cut here)
        const uint64_t slice0 = (uint64_t)blockIdx.x << t.log2_bucket;
        for (uint32_t i = threadIdx.x; i < n_slots; i += BLK) {
            const unsigned long long v = tab[i];
            uint32_t c = (uint32_t)(v & HASH_CMASK);
            if (c > HASH_SAT + (MASKED ? 1u : 0u)) c = HASH_SAT + (MASKED ? 1u : 0u);      // (MASKED: the slices keep the bias)
            gstore(t.slots, slice0 + i, 1ull << t.log2_slots, v ? (v & ~(unsigned long long)HASH_CMASK) | c : 0ull, status);
        }
        if (threadIdx.x == 0) wbeg[blockIdx.x] = wbase;
        return;
    }
    if (HALF) {
        // (also the LAST piece of an N-rank count half in pieces, accum 3 or 4: the bucket leaves what one count half leaves)
        // the bucket's occupied slots, in slot order: a bitmap of the occupancy (64 consecutive slots = the lanes of one wavefront:
        // a ballot), ranks from the popcounts of its words, the entries written to consecutive places (coalesced).  The LDS table
        // stays as it is until every slot has been read (the bitmap and its scan live behind it, where the rings were).
        unsigned long long *occ_l = tab + tab_units;             // [n_slots / 64] occupancy words, then as many exclusive ranks (uint32)
        const uint32_t n_occ = n_slots >= 64u ? n_slots >> 6 : 1u;
        uint32_t *rank_l = reinterpret_cast<uint32_t *>(occ_l + n_occ);
        __shared__ uint32_t n_entries;
        unsigned long long v[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t i = q * BLK + threadIdx.x;
            unsigned long long x = i < n_slots ? tab[i] : 0ull;
            const bool occupied = x != 0ull;
            if (x) {                                             // (the count stops at SAT; the overshoot of concurrent adds is clamped here)
                uint32_t c = (uint32_t)(x & HASH_CMASK) - (MASKED ? 1u : 0u);     // (MASKED: the bias off -- a row-only k-mer has count 0)
                if (c > HASH_SAT) c = HASH_SAT;
                x = (x & ~(unsigned long long)HASH_CMASK) | c;
            }
            v[q] = x;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(occupied);
            if (lane == 0 && q * BLK + wave * 64u < (n_slots >= 64u ? n_slots : 64u)) occ_l[(q * BLK + wave * 64u) >> 6] = m;
        }
        __syncthreads();
        if (threadIdx.x < 64) {                                  // exclusive ranks of the occupancy words (at most 256 of them), by one wavefront
            uint32_t run = 0;
            for (uint32_t w0 = 0; w0 < n_occ; w0 += 64) {
                const uint32_t wi = w0 + threadIdx.x;
                const uint32_t c = wi < n_occ ? (uint32_t)__popcll(occ_l[wi]) : 0u;
                uint32_t incl = c;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = __shfl_up(incl, d);
                    if ((int)threadIdx.x >= d) incl += o;
                }
                if (wi < n_occ) rank_l[wi] = run + incl - c;
                run += __shfl(incl, 63);
            }
            if (threadIdx.x == 0) n_entries = run;
        }
        __syncthreads();
        // (capacities for the checked build: the slabs of all buckets of this launch)
        const uint64_t ent0 = (uint64_t)blockIdx.x << t.log2_bucket, ent_cap = (uint64_t)gridDim.x << t.log2_bucket;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t i = q * BLK + threadIdx.x;
            if (i < n_slots && (MASKED ? ((occ_l[i >> 6] >> (i & 63u)) & 1ull) != 0ull : v[q] != 0ull)) {    // (MASKED: an entry may be 0)
                const unsigned long long m = occ_l[i >> 6];
                gstore(hv.ent, ent0 + rank_l[i >> 6] + (uint32_t)__popcll(m & ((1ull << (i & 63u)) - 1ull)), ent_cap, v[q], status);
            }
        }
        for (uint32_t wi = threadIdx.x; wi < n_occ; wi += BLK) gstore(hv.occ, (uint64_t)blockIdx.x * n_occ + wi, (uint64_t)gridDim.x * n_occ, occ_l[wi], status);
        if (threadIdx.x == 0) {
            hv.fill[blockIdx.x] = (long long)n_entries;
            hv.ring_cnt[blockIdx.x] = emitted_ring;
            wbeg[blockIdx.x] = wbase;
        }
        return;
    }
    if (emit_slots) {
        // the packed slice (an empty table needs no clearing: every slot is written), and the table shrinks to 2-byte bins:
        // 0 = slot never filled, 0xffff = bin out of range, else bin + 1.  (Every lane first reads all its slots -- the bins
        // land on top of the first quarter of the table.)
        uint16_t mybin[16];
        const float rcp_window = 1.0f / (float)window;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t i = q * BLK + threadIdx.x;
            mybin[q] = 0;
            if (i < n_slots) {
                const unsigned long long v = tab[i];
                uint32_t c;
                if (WIDE) {
                    c = cnts[i];
                    slice[i] = v;
                    slice_counts[i] = c;
                } else {
                    c = (uint32_t)(v & HASH_CMASK);
                    if (c > HASH_SAT) c = HASH_SAT;
                    slice[i] = v ? (v & ~(unsigned long long)HASH_CMASK) | c : 0ull;
                }
                const uint32_t bin = div_uniform(c, window, rcp_window);
                // (the merged lookups read the bin itself, 0xffff = none; the word-wise ones bin + 1, 0 = slot never filled)
                mybin[q] = MERGE ? (uint16_t)(v && bin < vsize ? bin : 0xffffu) : (uint16_t)(v ? (bin < vsize ? bin + 1u : 0xffffu) : 0u);
            }
        }
        __syncthreads();
        uint16_t *bins16 = reinterpret_cast<uint16_t *>(tab);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t i = q * BLK + threadIdx.x;
            if (i < n_slots) bins16[i] = mybin[q];
        }
        PG_STAMP(2);
        // ---- provisional (row, slot) words -> (row, bin) words, scattered at once by the first digit of their row group into
        // the row shuffle's regions (an LDS multisplit per tile of 16 Ki words, one global cursor add per digit and tile): the
        // final words never make a trip of their own through HBM
        unsigned char *lds = reinterpret_cast<unsigned char *>(tab);
        const uint32_t np = (uint32_t)n_lookups;
        if (MERGE) {
            MergeCtx mc;
            mc.lds = lds; mc.smask = smask; mc.vbits = vbits; mc.sh = sh; mc.status = status;
            mc.prov_b = prov_b; mc.meta_s = meta + r0; mc.meta_l = meta + rs; mc.n_s = (uint32_t)(rs - r0); mc.n_l = (uint32_t)(r1 - rs);
#ifdef PG_MINI_STAMPS
            mc.dbg = dbg;
#endif
            merged_lookup<CAP, BLK, DIG>(mc);
            PG_STAMP(3);
#ifdef PG_MINI_GAPS
            __syncthreads();
            if (threadIdx.x == 0 && n_short) {             // (n_short: there was a second pass, `bases` is buffer B)
                unsigned long long *gap = (unsigned long long *)(bases - rec_cap) + 4ull * blockIdx.x;     // (the first pass's buffer: dead by now)
                gap[0] = gap_t0;
                gap[1] = __builtin_amdgcn_s_memtime();
                gap[2] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);    // HW_ID, XCC_ID
                gap[3] = (unsigned long long)(r1 - r0);
            }
#endif
            return;
        }
        {
            WordCtx wc;
            wc.lds = lds; wc.smask = smask; wc.np = np; wc.lb = lb; wc.vbits = vbits; wc.sh = sh; wc.status = status; wc.prov_b = prov_b;
#ifdef PG_MINI_STAMPS
            wc.dbg = dbg;
#endif
            wordwise_lookup<BLK, DIG>(wc);
        }
        PG_STAMP(3);
        return;
    }
    // the packed slice (an empty table needs no clearing: every slot is written); then counts -> bins, in place
    const float rcp_window_g = window ? 1.0f / (float)window : 0.0f;
    for (uint32_t i = threadIdx.x; i < n_slots; i += BLK) {
        const unsigned long long v = tab[i];
        if (WIDE) {
            const uint32_t c = cnts[i];
            slice[i] = v;
            slice_counts[i] = c;
            if (window && v) {
                const uint32_t bin = div_uniform(c, window, rcp_window_g);
                cnts[i] = bin < vsize ? bin + 1u : BIN_NONE;
            }
            continue;
        }
        uint32_t c = (uint32_t)(v & HASH_CMASK);
        if (c > HASH_SAT) c = HASH_SAT;
        slice[i] = v ? (v & ~(unsigned long long)HASH_CMASK) | c : 0ull;
        if (window && v) {
            const uint32_t bin = div_uniform(c, window, rcp_window_g);
            tab[i] = (v & ~(unsigned long long)HASH_CMASK) | (bin < vsize ? bin + 1u : BIN_NONE);
        }
    }
    PG_STAMP(2);
    if (!window) return;
    // this bucket's words go to a range of the word buffer claimed with one global add: an upper bound, every k-mer inside a row
    if (threadIdx.x == 0) {
        wbase = atomicAdd(word_cursor, n_lookups);
        wbeg[blockIdx.x] = wbase;
    }
    __syncthreads();
    wb = wbase;
    // ---- general form: the records are read and probed a second time
    // (row, bin) words of 64 lanes -> the bucket's word range: one LDS add per call, the stores are contiguous
    auto emit = [&](bool put, uint32_t row, uint32_t bin1) {
        const unsigned long long pm = __ballot(put);
        if (pm) {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&emitted, (uint32_t)__popcll(pm));
            at = __shfl(at, 0);
            if (put) words[wb + at + lanes_below(pm)] = (row << vbits) | (bin1 - 1u);
        }
    };
    {
        head = tail = 0;
        int64_t i = r0 + (int64_t)wave * 64 + lane;
        uint64_t R = i < r1 ? bases[i] : 0ull;
        uint32_t m = i < r1 ? meta[i] : 0xffffffffu;
        for (int64_t i0 = r0 + (int64_t)wave * 64; i0 < r1; i0 += BLK) {
            const bool live = i0 + lane < r1;
            const uint32_t row = m >> META_ROW_SHIFT;
            const int n = live && row != MINI_ROW_NONE ? (int)((m >> META_D2_BITS) & (MINI_MAX_LEN - 1)) + 1 : 0;
            const uint64_t FW = rev2_64(R), RC = R ^ 0xAAAAAAAAAAAAAAAAull;
            i = i0 + BLK + lane;
            R = i < r1 ? bases[i] : 0ull;
            m = i < r1 ? meta[i] : 0xffffffffu;
            uint64_t code[CAP];
            unsigned long long cur[CAP];
            uint32_t bin1[CAP];                                  // count field of a k-mer found at its home slot: bin + 1, or BIN_NONE
#pragma unroll
            for (int j = 0; j < CAP; ++j) {
                const uint64_t fw = (FW >> (2 * j)) & kmask, rc = (RC >> (rc_sh0 - 2 * j)) & kmask;
                code[j] = fw < rc ? fw : rc;
                const uint32_t sl = mini_slot_hash<WIDE>(code[j]) & smask;
                cur[j] = j < n ? tab[sl] : 0ull;
                bin1[j] = WIDE ? (j < n ? cnts[sl] : 0u) : 0u;
            }
            // settled by the first probe: a hit (emit, unless its bin is out of range) or an empty slot (cannot happen for a
            // counted k-mer; nothing to emit).  Slot by slot, ONE add on the bucket's counter per batch.
            unsigned long long pm[CAP];
            uint32_t total = 0;
#pragma unroll
            for (int j = 0; j < CAP; ++j) {
                const bool hit = j < n && (WIDE ? cur[j] == code[j] + 1ull : cur[j] != 0 && (cur[j] >> HASH_CBITS) == code[j]);
                if (!WIDE) bin1[j] = (uint32_t)(cur[j] & HASH_CMASK);
                pm[j] = __ballot(hit && bin1[j] != BIN_NONE);
                total += (uint32_t)__popcll(pm[j]);
            }
#ifdef PG_MINI_STAMPS
            {   // how many words would be left if equal neighbouring words of a record travelled as one (dbg[10] words, dbg[11] runs)
                uint32_t nw = 0, nr = 0;
#pragma unroll
                for (int j = 0; j < CAP; ++j) {
                    const bool wj = (pm[j] >> lane) & 1ull;
                    const bool same = j > 0 && ((pm[j > 0 ? j - 1 : 0] >> lane) & 1ull) && bin1[j] == bin1[j > 0 ? j - 1 : 0];
                    nw += wj;
                    nr += wj && !same;
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) { nw += __shfl_down(nw, d); nr += __shfl_down(nr, d); }
                if (lane == 0) { atomicAdd(&dbg[10], (unsigned long long)nw); atomicAdd(&dbg[11], (unsigned long long)nr); }
            }
#endif
            if (total) {                                         // (uniform)
                uint32_t at = 0;
                if (lane == 0) at = atomicAdd(&emitted, total);
                at = __shfl(at, 0);
#pragma unroll
                for (int j = 0; j < CAP; ++j) {
                    if ((pm[j] >> lane) & 1ull) words[wb + at + lanes_below(pm[j])] = (row << vbits) | (bin1[j] - 1u);
                    at += (uint32_t)__popcll(pm[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < CAP; ++j) {                      // collisions: onto the ring
                const bool pend = j < n && cur[j] != 0 && (WIDE ? cur[j] != code[j] + 1ull : (cur[j] >> HASH_CBITS) != code[j]);
                const unsigned long long mask = __ballot(pend);
                if (mask) {
                    if (pend) {
                        const uint32_t at = (tail + lanes_below(mask)) & (RING - 1);
                        ring[at] = code[j];
                        ring_row[at] = row;
                    }
                    tail += (uint32_t)__popcll(mask);
                    if (tail - head >= 64) {
                        const uint32_t at = (head + lane) & (RING - 1);
                        const uint64_t c = ring[at];
                        const uint32_t rw = ring_row[at];
                        head += 64;
                        const uint32_t b1 = mini_lookup_slow<WIDE>(tab, cnts, smask, limit, c, true);
                        emit(b1 != BIN_NONE, rw, b1);
                    }
                }
            }
        }
        if (tail != head) {
            const bool act = lane < tail - head;
            const uint32_t at = (head + lane) & (RING - 1);
            const uint64_t c = act ? ring[at] : 0ull;
            const uint32_t rw = act ? ring_row[at] : 0u;
            const uint32_t b1 = mini_lookup_slow<WIDE>(tab, cnts, smask, limit, c, act);
            emit(b1 != BIN_NONE, rw, b1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) emit_end[blockIdx.x] = wb + emitted;
}

// ---- N > 1 ranks: the other kernels of the super-k-mer form (pangaea_amd/dist.py: features_sharded_mini)
//
// rank:   plan -> A1' -> A2' -> mini_count_kernel<..., HALF>     entries + occupancy per bucket, provisional words
//         mini_gather_entries_kernel                              entries, bucket-ordered, into the send buffer (owner ranges)
//         ---- all-to-all: every bucket range to its owner (8 bytes per entry)
// owner:  mini_merge_bins_kernel                                  per owned bucket: the N parts summed inside LDS -> its slice of the
//                                                                 global table, and for EVERY entry received its bin (2 bytes), in order
//         ---- all-to-all back (2 bytes per entry)
// rank:   mini_lookup_half_kernel                                 bins + occupancy -> the bucket's 2-byte bins in LDS -> lookups of the
//                                                                 provisional words (as the one-GPU kernel does), row-group scatter
__global__ __launch_bounds__(BLOCK) void mini_gather_entries_kernel(const unsigned long long *__restrict__ ent, int log2_bucket,
                                                                    const long long *__restrict__ fill, const long long *__restrict__ dst_elem,
                                                                    unsigned long long *__restrict__ out, unsigned long long out_cap, uint32_t *status)
{
    const unsigned long long *src = ent + ((uint64_t)blockIdx.x << log2_bucket);
    const long long n = fill[blockIdx.x], d0 = dst_elem[blockIdx.x];
    for (long long i = threadIdx.x; i < n; i += BLOCK) gstore(out, (uint64_t)(d0 + i), out_cap, src[i], status);
}

// one workgroup per OWNED bucket: part p's entries of owned bucket i lie at recv[p * part_stride + seg[p * (n_owned + 1) + i] ..
// seg[... + i + 1]) (slot format: canonical code << 22 | count, counts <= SAT); bins_out has the same layout in uint16:
// bin + 1 of the entry's k-mer in the MERGED table, 0xffff when the bin lies beyond the vector.
// MASKED (pg_mini_merge_bins_masked): an entry of count 0 (a k-mer that only rows of its sender saw: pg_mini_count_half_masked) is
// not inserted: once every counted entry is in, it is LOOKED UP -- its slot if some rank counted the k-mer, else no bin (0xffff).
// The slices then hold counted k-mers only: no zero entries, no holes in probe chains (count_kmer.cpp:87 skips what the dump lacks).
template <bool MASKED = false>
__global__ __launch_bounds__(BIG_BLOCK) void mini_merge_bins_kernel(const unsigned long long *__restrict__ recv, long long part_stride,
                                                                    const long long *__restrict__ seg, int n_parts, int n_owned,
                                                                    MiniView t, long long bucket0, uint32_t window, uint32_t vsize,
                                                                    uint16_t *__restrict__ bins_out, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    const uint32_t n_slots = 1u << t.log2_bucket, smask = n_slots - 1u;
    const uint32_t limit = n_slots < MAX_PROBE ? n_slots : MAX_PROBE;
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) tab[i] = 0ull;
    __syncthreads();
    bool full = false;
    // Insert: four entries of the lane in flight (their loads, then their first probes, issued together); the slot an entry ends up
    // in is left where its bin will go -- the second sweep then needs neither the entry nor its hash nor a probe, only the slot's
    // final count (until round 4 it read the 8-byte entries again and probed again: 3.16 ms for the 8-rank geometry)
    constexpr int U = 4;
    const uint64_t out_cap = (uint64_t)n_parts * (uint64_t)part_stride;
    for (int p = 0; p < n_parts; ++p) {
        const long long a = seg[(long long)p * (n_owned + 1) + blockIdx.x], b = seg[(long long)p * (n_owned + 1) + blockIdx.x + 1];
        for (long long e0 = a + threadIdx.x; e0 < b; e0 += (long long)U * BIG_BLOCK) {
            unsigned long long x[U], cur[U];
            uint32_t s[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long e = e0 + (long long)u * BIG_BLOCK;
                x[u] = e < b ? recv[(long long)p * part_stride + e] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = mini_slot_hash<false>(x[u] >> HASH_CBITS) & smask;
                cur[u] = tab[s[u]];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long e = e0 + (long long)u * BIG_BLOCK;
                if (e >= b) continue;
                const uint64_t code = x[u] >> HASH_CBITS;
                const uint32_t c = (uint32_t)(x[u] & HASH_CMASK);
                if (MASKED && c == 0u) continue;                 // (looked up below)
                uint32_t at = s[u];
                unsigned long long cv = cur[u];
                bool done = false;
                for (uint32_t i = 0; i < limit && !done; ++i) {
                    if (i) cv = tab[at];
                    if (cv == 0ull) {
                        cv = atomicCAS(&tab[at], 0ull, x[u]);
                        if (cv == 0ull) { done = true; break; }
                    }
                    if ((cv >> HASH_CBITS) == code) {            // add, saturating: parts of up to SAT each must not carry into the code
                        for (;;) {
                            const uint32_t sum = (uint32_t)(cv & HASH_CMASK) + c;
                            const unsigned long long nv = (cv & ~(unsigned long long)HASH_CMASK) | (sum > HASH_SAT ? HASH_SAT : sum);
                            const unsigned long long old = atomicCAS(&tab[at], cv, nv);
                            if (old == cv) break;
                            cv = old;
                        }
                        done = true;
                        break;
                    }
                    at = (at + 1) & smask;
                }
                full |= !done;
                // (a k-mer that found no place -- the table is full and reported so -- has no slot and no bin)
                gstore(bins_out, (uint64_t)((long long)p * part_stride + e), out_cap, (uint16_t)(done ? at : 0xffffu), status);
            }
        }
    }
    if (full) atomicOr(status, PG_STATUS_TABLE_FULL);
    __syncthreads();
    if constexpr (MASKED) {
        // the count-0 entries: found or not, nothing is inserted (every lane again treats the entries it treated above)
        for (int p = 0; p < n_parts; ++p) {
            const long long a = seg[(long long)p * (n_owned + 1) + blockIdx.x], b = seg[(long long)p * (n_owned + 1) + blockIdx.x + 1];
            for (long long e = a + threadIdx.x; e < b; e += BIG_BLOCK) {
                const unsigned long long x = recv[(long long)p * part_stride + e];
                if ((x & HASH_CMASK) != 0ull) continue;
                const uint64_t code = x >> HASH_CBITS;
                uint32_t at = mini_slot_hash<false>(code) & smask, found = 0xffffu;
                for (uint32_t i = 0; i < limit; ++i) {
                    const unsigned long long cv = tab[at];
                    if (cv == 0ull) break;
                    if ((cv >> HASH_CBITS) == code) { found = at; break; }
                    at = (at + 1) & smask;
                }
                gstore(bins_out, (uint64_t)((long long)p * part_stride + e), out_cap, (uint16_t)found, status);
            }
        }
    }
    const uint64_t slice0 = (uint64_t)(bucket0 + blockIdx.x) << t.log2_bucket;
    for (uint32_t i = threadIdx.x; i < n_slots; i += BIG_BLOCK) gstore(t.slots, slice0 + i, 1ull << t.log2_slots, tab[i], status);
    // slots -> bins (every lane reads back what it wrote itself: the same entries in the same order)
    const float rcp_window = 1.0f / (float)window;
    for (int p = 0; p < n_parts; ++p) {
        const long long a = seg[(long long)p * (n_owned + 1) + blockIdx.x], b = seg[(long long)p * (n_owned + 1) + blockIdx.x + 1];
        for (long long e0 = a + threadIdx.x; e0 < b; e0 += (long long)U * BIG_BLOCK) {
            uint32_t sl[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long e = e0 + (long long)u * BIG_BLOCK;
                sl[u] = e < b ? (uint32_t)bins_out[(long long)p * part_stride + e] : 0xffffu;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long e = e0 + (long long)u * BIG_BLOCK;
                if (e >= b) continue;
                uint32_t out = 0xffffu;
                if (sl[u] != 0xffffu) {
                    const uint32_t bin = div_uniform((uint32_t)(tab[sl[u] & smask] & HASH_CMASK), window, rcp_window);
                    out = bin < vsize ? bin + 1u : 0xffffu;
                }
                gstore(bins_out, (uint64_t)((long long)p * part_stride + e), out_cap, (uint16_t)out, status);
            }
        }
    }
}

// (the word-wise lookups; the merged form -- merged_lookup with the hit planes of a MERGE count half -- plugs in here once it
// is the faster one)
template <int BLK, int DIG>
__global__ __launch_bounds__(BLK, 4) void mini_lookup_half_kernel(const unsigned long long *__restrict__ kwords, const unsigned long long *__restrict__ wbeg,
                                                                const unsigned long long *__restrict__ occ,
                                                                const uint16_t *__restrict__ bins_in, const long long *__restrict__ bin_elem,
                                                                int log2_bucket, int vbits, const uint32_t *__restrict__ prov, ShufArgs sh, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    if (*status & PG_STATUS_OVERFLOW_LIST) return;               // (the exchange did not take place: dist.MiniSharded.exchange; no bins to read)
    const uint32_t n_slots = 1u << log2_bucket, smask = n_slots - 1u;
    const uint32_t n_occ = n_slots >= 64u ? n_slots >> 6 : 1u;
    const uint32_t np_all = (uint32_t)kwords[blockIdx.x];
    if (np_all == 0u) return;                                    // (uniform: no k-mer of this bucket lies inside a row)
    // the bucket's 2-byte bins: slot i holds the entry of rank (occupied slots below i), whose bin came back in that order.
    // Occupancy words and their exclusive ranks go to LDS first (behind the bins and the lookup's areas: the tail of the tile
    // buffer, which the lookups only use later), two barriers in all
    uint16_t *bins16 = reinterpret_cast<uint16_t *>(lds);
    const uint16_t *bi = bins_in + bin_elem[blockIdx.x];
    unsigned long long *occ_l = reinterpret_cast<unsigned long long *>(lds + LookupLds<BLK, DIG>::BUF);          // [n_occ] words, then [n_occ] ranks
    uint32_t *rank_l = reinterpret_cast<uint32_t *>(occ_l + n_occ);
    for (uint32_t wi = threadIdx.x; wi < n_occ; wi += BLK) occ_l[wi] = occ[(uint64_t)blockIdx.x * n_occ + wi];
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t run = 0;
        for (uint32_t w0 = 0; w0 < n_occ; w0 += 64) {
            const uint32_t wi = w0 + threadIdx.x;
            const uint32_t c = wi < n_occ ? (uint32_t)__popcll(occ_l[wi]) : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)threadIdx.x >= d) incl += o;
            }
            if (wi < n_occ) rank_l[wi] = run + incl - c;
            run += __shfl(incl, 63);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += BLK) {
        const unsigned long long m = occ_l[i >> 6];
        bins16[i] = (m >> (i & 63u)) & 1ull ? bi[rank_l[i >> 6] + (uint32_t)__popcll(m & ((1ull << (i & 63u)) - 1ull))] : (uint16_t)0;
    }
    __syncthreads();
    WordCtx wc;
    wc.lds = lds; wc.smask = smask; wc.np = np_all; wc.lb = log2_bucket; wc.vbits = vbits; wc.sh = sh; wc.status = status;
    wc.prov_b = prov + wbeg[blockIdx.x];
    wc.dbg = nullptr;
    wordwise_lookup<BLK, DIG>(wc);
}

// the merged form of the lookup half: the count half left its provisional words in fixed slots (MergeArgs).  PIECE (a count half
// in pieces, pg_mini_lookup_half_piece): off / n_short / wbeg / mprov / meta are ONE piece's, and a bucket without records of
// that piece leaves at once (as mini_lookup_slice_merge_kernel does)
template <int CAP, int BLK, int DIG, bool PIECE = false>
__global__ __launch_bounds__(BLK, 4) void mini_lookup_half_merge_kernel(const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ n_short,
                                                                      const unsigned long long *__restrict__ wbeg, const uint32_t *__restrict__ ring_cnt,
                                                                      const unsigned long long *__restrict__ occ,
                                                                      const uint16_t *__restrict__ bins_in, const long long *__restrict__ bin_elem,
                                                                      int log2_bucket, int vbits, const uint32_t *__restrict__ mprov,
                                                                      const uint32_t *__restrict__ meta, ShufArgs sh, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    if (*status & PG_STATUS_OVERFLOW_LIST) return;               // (the exchange did not take place: dist.MiniSharded.exchange; no bins to read)
    const uint32_t n_slots = 1u << log2_bucket, smask = n_slots - 1u;
    const uint32_t n_occ = n_slots >= 64u ? n_slots >> 6 : 1u;
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (PIECE && r1 == r0) return;                               // (uniform: the piece has no record of this bucket)
    const int64_t rs = n_short && CAP > SHORT_MAX ? r0 + (int64_t)n_short[blockIdx.x] : r0;
    uint16_t *bins16 = reinterpret_cast<uint16_t *>(lds);
    const uint16_t *bi = bins_in + bin_elem[blockIdx.x];
    unsigned long long *occ_l = reinterpret_cast<unsigned long long *>(lds + MergeLds<BLK, DIG>::BUF);          // [n_occ] words, then [n_occ] ranks
    uint32_t *rank_l = reinterpret_cast<uint32_t *>(occ_l + n_occ);
    for (uint32_t wi = threadIdx.x; wi < n_occ; wi += BLK) occ_l[wi] = occ[(uint64_t)blockIdx.x * n_occ + wi];
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t run = 0;
        for (uint32_t w0 = 0; w0 < n_occ; w0 += 64) {
            const uint32_t wi = w0 + threadIdx.x;
            const uint32_t c = wi < n_occ ? (uint32_t)__popcll(occ_l[wi]) : 0u;
            uint32_t incl = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = __shfl_up(incl, d);
                if ((int)threadIdx.x >= d) incl += o;
            }
            if (wi < n_occ) rank_l[wi] = run + incl - c;
            run += __shfl(incl, 63);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_slots; i += BLK) {
        const unsigned long long m = occ_l[i >> 6];
        // (what travels is bin + 1, 0xffff = beyond the vector; merged_lookup reads the bin itself, 0xffff = none)
        const uint16_t x = (m >> (i & 63u)) & 1ull ? bi[rank_l[i >> 6] + (uint32_t)__popcll(m & ((1ull << (i & 63u)) - 1ull))] : (uint16_t)0;
        bins16[i] = (uint16_t)(x != 0 && x != 0xffffu ? x - 1u : 0xffffu);
    }
    __syncthreads();
    MergeCtx mc;
    mc.lds = lds; mc.smask = smask; mc.vbits = vbits; mc.sh = sh; mc.status = status;
    mc.prov_b = mprov + wbeg[blockIdx.x];
    mc.meta_s = meta + r0; mc.meta_l = meta + rs; mc.n_s = (uint32_t)(rs - r0); mc.n_l = (uint32_t)(r1 - rs);
    mc.dbg = nullptr;
    merged_lookup<CAP, BLK, DIG>(mc);
}

// PIECES: the lookups of ONE piece's provisional slots in the final table -- the bucket's slice becomes its 2-byte bins in LDS
// (as the fused kernel makes them), then merged_lookup on the piece's slots and the kept meta words of its records
template <int CAP, int BLK, int DIG>
__global__ __launch_bounds__(BLK, 4) void mini_lookup_slice_merge_kernel(const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ n_short,
                                                                       const unsigned long long *__restrict__ wbeg, MiniView t, uint32_t window, uint32_t vsize,
                                                                       int vbits, const uint32_t *__restrict__ mprov, const uint32_t *__restrict__ meta,
                                                                       ShufArgs sh, uint32_t *status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t n_slots = 1u << t.log2_bucket, smask = n_slots - 1u;
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (r1 == r0) return;                                        // (uniform: the piece has no record of this bucket)
    const int64_t rs = n_short && CAP > SHORT_MAX ? r0 + (int64_t)n_short[blockIdx.x] : r0;
    uint16_t *bins16 = reinterpret_cast<uint16_t *>(lds);
    const uint64_t *slice = t.slots + ((uint64_t)blockIdx.x << t.log2_bucket);
    const float rcp_window = 1.0f / (float)window;
    for (uint32_t i = threadIdx.x; i < n_slots; i += BLK) {
        const unsigned long long v = slice[i];
        const uint32_t bin = div_uniform((uint32_t)(v & HASH_CMASK), window, rcp_window);
        bins16[i] = (uint16_t)(v && bin < vsize ? bin : 0xffffu);        // (merged_lookup reads the bin itself, 0xffff = none)
    }
    __syncthreads();
    MergeCtx mc;
    mc.lds = lds; mc.smask = smask; mc.vbits = vbits; mc.sh = sh; mc.status = status;
    mc.prov_b = mprov + wbeg[blockIdx.x];
    mc.meta_s = meta + r0; mc.meta_l = meta + rs; mc.n_s = (uint32_t)(rs - r0); mc.n_l = (uint32_t)(r1 - rs);
    mc.dbg = nullptr;
    merged_lookup<CAP, BLK, DIG>(mc);
}

// ---- FIND (pg_mini_find): the bucket workgroup that finds instead of inserting -- abundance rows against a FINISHED table
// (count_kmer -g DUMP, cpptools/count_kmer.cpp:55-108; a k-mer the table lacks adds nothing, :87).  The records are those of
// any stream, delivered bucket by bucket by the plan and the two scatter passes as for a count; the table is only read.
//   1  the bucket's slice of the given table -> LDS (16-byte loads), the bucket's range of the MERGE layout claimed
//   2  every record that lies in a row is expanded as the count loop does and each k-mer walks its chain read-only: home slot,
//      linear, wrapping inside the bucket, until its key or an empty slot, at most `limit` steps; the slot where the walk ended
//      goes to the k-mer's fixed halfword (MergeArgs).  An empty slot's bin reads 0xffff, which is what an absent k-mer needs.
//   3  slots -> 2-byte bins at the start of the dynamic LDS, merged_lookup as in the fused kernel.
// A walk that sees `limit` = all slots of the bucket without its key or an empty one (an absent k-mer in a bucket without a free
// slot) leaves halfword n_slots: the bins area has room for that entry (set to 0xffff) wherever the bucket is smaller than the
// area.  Where it is not (2^13 slots on 512 threads, 2^14 on 1024) the bucket writes nothing and sets PG_STATUS_TABLE_FULL:
// the caller takes the lookup form (KmerTable.abundance_of).
template <int CAP, int BLK, int DIG>
__global__ __launch_bounds__(BLK, 4) void mini_find_kernel(const uint64_t *__restrict__ bases, const uint32_t *__restrict__ meta,
                                                              const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ n_short,
                                                              MiniView t, uint32_t window, uint32_t vsize, int vbits,
                                                              unsigned long long *__restrict__ word_cursor, ShufArgs sh, MergeArgs mg,
                                                              unsigned long long rec_cap, uint32_t *status)
{
    // (a plan of another stream: see mini_count_kernel)
    if (word_cursor[-1] > rec_cap || (*status & PG_STATUS_PLAN_MISMATCH)) {
        if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, PG_STATUS_PLAN_MISMATCH);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned long long tab[];
    __shared__ unsigned long long wbase;
    __shared__ uint32_t no_room;                                 // some absent k-mer saw every slot of the bucket taken
    const uint32_t n_slots = 1u << t.log2_bucket, smask = n_slots - 1u;
    const uint32_t limit = n_slots < MAX_PROBE ? n_slots : MAX_PROBE;
    const int64_t r0 = (int64_t)off[blockIdx.x], r1 = (int64_t)off[blockIdx.x + 1];
    if (r1 == r0) return;                                        // (uniform: no record of this bucket)
    const int64_t rs = n_short && CAP > SHORT_MAX ? r0 + (int64_t)n_short[blockIdx.x] : r0;
    const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
    const int rc_sh0 = 2 * (32 - t.k);
    constexpr uint32_t CXS_ = CAP > SHORT_MAX ? SHORT_MAX : CAP;
    const uint32_t n_sb = (uint32_t)((rs - r0 + 63) >> 6), n_lb = (uint32_t)((r1 - rs + 63) >> 6);
    // ---- 1: the slice (two slots per load; a bucket has at least 16), the bucket's range of fixed places (dwords; see MergeArgs)
    {
        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(t.slots + ((uint64_t)blockIdx.x << t.log2_bucket));
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(tab);
        for (uint32_t i = threadIdx.x; i < n_slots / 2; i += BLK) dst[i] = src[i];
    }
    const unsigned long long fixed_words = 32ull * n_sb * CXS_ + 32ull * n_lb * CAP;
    if (threadIdx.x == 0) { wbase = atomicAdd(word_cursor, fixed_words); no_room = 0; }
    __syncthreads();
    {
        const unsigned long long need = fixed_words + (unsigned long long)MergeStep<CAP>::SLACK;
        if (wbase + need > mg.cap || 2ull * need >= (unsigned long long)RING_NOPLACE) {      // (uniform; a plan of other reads, as in mini_count_kernel)
            if (threadIdx.x == 0) atomicOr(status, PG_STATUS_PLAN_MISMATCH);
            return;
        }
    }
    const unsigned long long wb = ((unsigned long long)uniform32((uint32_t)(wbase >> 32)) << 32) | uniform32((uint32_t)wbase);
    uint32_t *const prov_b = mg.prov + wb;
    uint16_t *const prov_h = reinterpret_cast<uint16_t *>(prov_b);
    const uint32_t long_base = n_sb * 64u * CXS_;                // (halfwords)
    const uint32_t np_half = long_base + n_lb * 64u * CAP;
    // ---- 2: wavefront w takes the batches [ra + 64 (w + BLK / 64 t), + 64) of a class; CX = k-mers per record at most there
    bool lost = false;
    auto find_range = [&](auto cx, int64_t ra, int64_t rb) {
        constexpr int CX = decltype(cx)::value;
        for (int64_t i0 = ra + (int64_t)wave * 64; i0 < rb; i0 += BLK) {
            const bool live = i0 + lane < rb;
            const uint64_t R = live ? bases[i0 + lane] : 0ull;
            const uint32_t m = live ? meta[i0 + lane] : 0xffffffffu;
            // (a record outside every row is looked up by nobody: merged_lookup skips its halfwords)
            const int n = (m >> META_ROW_SHIFT) != MINI_ROW_NONE ? (int)((m >> META_D2_BITS) & (MINI_MAX_LEN - 1)) + 1 : 0;
            if (!__any(n > 0)) continue;                         // (uniform)
            const uint32_t place0 = (CX < CAP ? 0u : long_base) + (uint32_t)((i0 - ra) >> 6) * (64u * CX) + lane;
            const uint64_t FW = rev2_64(R), RC = R ^ 0xAAAAAAAAAAAAAAAAull;
            uint64_t code[CX];
            uint32_t sl[CX];
            unsigned long long cur[CX];
#pragma unroll
            for (int j = 0; j < CX; ++j) {                       // the home slots of the record's k-mers, all reads in flight
                const uint64_t fw = FW << ((rc_sh0 - 2 * j) & 63), rc = RC << (2 * j);        // (as the count loop: j beyond n selects some slot, read and ignored)
                code[j] = (fw < rc ? fw : rc) >> rc_sh0;
                sl[j] = mini_slot_hash<false>(code[j]) & smask;
                cur[j] = tab[sl[j]];
            }
#pragma unroll
            for (int j = 0; j < CX; ++j) {
                uint32_t s = sl[j], res = n_slots;
                bool todo = j < n;
                // one slot of the chain: the walk ends at the k-mer's own slot or at an empty one
                auto visit = [&](unsigned long long c) { if (todo && (c == 0ull || (c >> HASH_CBITS) == code[j])) { res = s; todo = false; } };
                visit(cur[j]);
                // (a lane walks its own chain; the round ends with the longest one, after `limit` slots at the latest)
                for (uint32_t q = 1; q < limit && __any(todo); ++q) {
                    s = (s + 1u) & smask;
                    visit(tab[s]);
                }
                lost |= todo;
                if (j < n) gstore(prov_h, (uint64_t)place0 + 64u * j, (uint64_t)np_half, (uint16_t)res, status);
            }
        }
    };
    find_range(std::integral_constant<int, (CAP > SHORT_MAX ? SHORT_MAX : CAP)>{}, r0, rs);
    find_range(std::integral_constant<int, CAP>{}, rs, r1);
    if (lost) atomicOr(&no_room, 1u);
    __syncthreads();                                             // (the last probe of the bucket is done: the slots may go)
    const bool spare = 2u * (n_slots + 1u) <= MergeLds<BLK, DIG>::BUF;           // (the bins area holds one entry more than the bucket has slots)
    if (no_room && !spare) {                                     // (uniform)
        if (threadIdx.x == 0) atomicOr(status, PG_STATUS_TABLE_FULL);
        return;
    }
    // ---- 3: the 2-byte bins (every lane reads all its slots first: the bins land on top of the first quarter of the slots)
    uint16_t mybin[16];
    const float rcp_window = 1.0f / (float)window;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t i = q * BLK + threadIdx.x;
        mybin[q] = 0xffffu;
        if (i < n_slots) {
            const unsigned long long v = tab[i];
            const uint32_t bin = div_uniform((uint32_t)(v & HASH_CMASK), window, rcp_window);
            mybin[q] = (uint16_t)(v && bin < vsize ? bin : 0xffffu);        // (merged_lookup reads the bin itself, 0xffff = none)
        }
    }
    __syncthreads();
    uint16_t *bins16 = reinterpret_cast<uint16_t *>(tab);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const uint32_t i = q * BLK + threadIdx.x;
        if (i < n_slots) bins16[i] = mybin[q];
    }
    if (spare && threadIdx.x == 0) bins16[n_slots] = 0xffffu;    // (what a walk without an end left)
    __syncthreads();
    MergeCtx mc;
    mc.lds = reinterpret_cast<unsigned char *>(tab); mc.smask = smask; mc.vbits = vbits; mc.sh = sh; mc.status = status;
    mc.prov_b = prov_b;
    mc.meta_s = meta + r0; mc.meta_l = meta + rs; mc.n_s = (uint32_t)(rs - r0); mc.n_l = (uint32_t)(r1 - rs);
    mc.dbg = nullptr;
    merged_lookup<CAP, BLK, DIG>(mc);
}

// ---- workspace of the plan: header | region_tot | region_off | off | hist | cur2 | cur2l | kwords | wbeg | round_row | chunk table
struct MiniPlan {
    int bits, bits1, bits2;
    int64_t n_rounds, n_chunks, chunk_stride;
    size_t header_off, rtot_off, roff_off, hist_off, off_off, cur2_off, cur2l_off, kw_off, wbeg_off, round_off, chunk_off, total;
};

// k-mers per record at most: what fits the 32 characters of a record and the 4-bit length field -- and the window: a
// minimizer covers at most W = k - M + 1 consecutive k-mers, so longer runs only exist where the same hashed M-mer recurs
// (homopolymers, short tandem repeats).  The bucket workgroups treat every record in `cap` unrolled, predicated steps: cutting
// those rare runs at W costs a few records and saves a quarter of the steps (k = 21: 12 -> 9; mini_count 19.1 -> 18.5 ms).
// PG_MINI_CAP overrides (tuning).
static_assert(MINI_MAX_WINDOW <= 9, "count kernels are instantiated for up to 9 k-mers per record");
int mini_cap(int k)
{
    int wc, woff;
    mini_window(k, &wc, &woff);
    int cap = 33 - k < MINI_MAX_LEN ? 33 - k : MINI_MAX_LEN;
    if (wc < cap) cap = wc;
    static const int forced = getenv("PG_MINI_CAP") ? atoi(getenv("PG_MINI_CAP")) : 0;
    if (forced >= 1 && forced < cap) cap = forced;
    return cap;
}
// the cap the bucket kernels are instantiated for (cap <= W <= 9: see mini_cap)
constexpr int cap_class(int cap) { return cap <= 4 ? 4 : cap <= 6 ? 6 : cap <= 8 ? 8 : 9; }

int check_mini(const pg_table *t, const char *who)
{
    if (!t || !t->data) return pg_fail(PG_EINVAL, "%s: table descriptor is null", who);
    if (t->kind != PG_TABLE_MINI && t->kind != PG_TABLE_MINI_WIDE) return pg_fail(PG_EINVAL, "%s: needs a PG_TABLE_MINI or PG_TABLE_MINI_WIDE table", who);
    const bool wide = t->kind == PG_TABLE_MINI_WIDE;
    const int k_lo = wide ? PG_HASH_MAX_K + 1 : PG_MINI_MIN_K, k_hi = wide ? PG_WIDE_MAX_K : PG_HASH_MAX_K;
    if (t->k < k_lo || t->k > k_hi) return pg_fail(PG_EINVAL, "%s: %s tables need %d <= k <= %d (got %d)", who, wide ? "wide mini" : "mini", k_lo, k_hi, t->k);
    const int lb_hi = wide ? PG_MINI_WIDE_MAX_LOG2_BUCKET_SLOTS : PG_BUCKET_MAX_LOG2_SLOTS;
    if (t->log2_bucket_slots < 4 || t->log2_bucket_slots > lb_hi)
        return pg_fail(PG_EINVAL, "%s: log2_bucket_slots %d out of range [4,%d]", who, t->log2_bucket_slots, lb_hi);
    const int bits = t->log2_slots - t->log2_bucket_slots;
    if (bits < 0 || bits > PG_MINI_MAX_LOG2_BUCKETS) return pg_fail(PG_EINVAL, "%s: 2^%d buckets (at most 2^%d)", who, bits, PG_MINI_MAX_LOG2_BUCKETS);
    return PG_OK;
}

int plan_mini(const pg_table *t, int64_t n_words, MiniPlan *p)
{
    p->bits = t->log2_slots - t->log2_bucket_slots;
    p->bits1 = p->bits < MINI_BITS1 ? p->bits : MINI_BITS1;
    if (p->bits - p->bits1 > META_D2_BITS) p->bits1 = p->bits - META_D2_BITS;       // (cannot happen: at most 2^16 buckets)
    p->bits2 = p->bits - p->bits1;
    p->n_rounds = (n_words + ROUND_WORDS - 1) / ROUND_WORDS;
    p->n_chunks = (n_words + MINI_CHUNK_WORDS - 1) / MINI_CHUNK_WORDS;
    if (p->n_chunks < 1) p->n_chunks = 1;
    // golden-ratio stride, made coprime to the chunk count: regions hold the stream in scrambled chunk order, so the bucket
    // workgroups (and the row shuffle behind them) do not all see the same rows at the same time
    p->chunk_stride = (int64_t)((double)p->n_chunks * 0.6180339887) | 1;
    auto gcd = [](int64_t a, int64_t b) { while (b) { int64_t r = a % b; a = b; b = r; } return a; };
    while (gcd(p->chunk_stride, p->n_chunks) != 1) p->chunk_stride += 2;
    const size_t nb = (size_t)1 << p->bits;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    p->header_off = take(512);
    p->rtot_off = take(((size_t)1 << MINI_MAX_BITS1) * 8);          // plan: records per region
    p->roff_off = take((((size_t)1 << MINI_MAX_BITS1) + 1) * 8);    // plan: where every region starts
    p->off_off = take((nb + 1) * 8);                                // count: where every bucket starts
    p->hist_off = take(nb * 8);                                     // count: records per bucket (cleared with the cursors behind it)
    p->cur2_off = take(nb * 8);
    p->cur2l_off = take(nb * 8);
    p->kw_off = take(nb * 8);
    p->wbeg_off = take(nb * 8);
    p->round_off = take((size_t)(p->n_rounds + 1) * 4);
    p->chunk_off = take(((size_t)p->n_chunks << p->bits1) * 8);
    p->total = o;
    return PG_OK;
}

// ---- one view per workspace: typed pointers, built by the one function that knows the layout and checks size and alignment (`who`:
// the entry point, for the message).  The const flavours serve the lookup entries, which read what a count left: they check the size only.
template <bool CONST, class T> using ws_ptr = std::conditional_t<CONST, const T, T> *;
bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 255) != 0; }

template <bool CONST> struct PlanViewT : MiniPlan {
    using Words = ws_ptr<CONST, unsigned long long>;
    Words header, region_tot, region_off, off, hist, cur2, cur2l, kwords, wbeg, chunk_tab;       // (header first; hist | cur2 | cur2l | kwords in a row)
    ws_ptr<CONST, int32_t> round_row;
    // short records per bucket, where the classes are sorted apart (the second scatter pass does that: without it -- at most 256
    // buckets -- every record counts as long)
    const unsigned long long *n_short(int k) const { return bits2 && mini_cap(k) > SHORT_MAX ? cur2 : nullptr; }
};
using PlanView = PlanViewT<false>; using ConstPlanView = PlanViewT<true>;

// false: plan_ws_bytes are too few for the plan of n_words words (nothing is carved then)
template <bool CONST> bool plan_carve(const pg_table *t, int64_t n_words, ws_ptr<CONST, void> plan_ws, int64_t plan_ws_bytes, PlanViewT<CONST> *v)
{
    plan_mini(t, n_words, v);
    if ((int64_t)v->total > plan_ws_bytes) return false;
    const auto ws = (ws_ptr<CONST, char>)plan_ws;
    auto words = [&](size_t at) { return (typename PlanViewT<CONST>::Words)(ws + at); };
    v->header = words(v->header_off); v->region_tot = words(v->rtot_off); v->region_off = words(v->roff_off); v->off = words(v->off_off);
    v->hist = words(v->hist_off); v->cur2 = words(v->cur2_off); v->cur2l = words(v->cur2l_off); v->kwords = words(v->kw_off);
    v->wbeg = words(v->wbeg_off); v->chunk_tab = words(v->chunk_off); v->round_row = (ws_ptr<CONST, int32_t>)(ws + v->round_off);
    return true;
}

// the workspace a plan or a count writes.  several: the entry point takes other workspaces too, and its messages say so
int plan_view(const pg_table *t, int64_t n_words, void *plan_ws, int64_t plan_ws_bytes, const char *who, bool several, PlanView *v)
{
    if (!plan_carve(t, n_words, plan_ws, plan_ws_bytes, v))
        return pg_fail(PG_EINVAL, several ? "%s: plan workspace of %lld bytes, %lld needed" : "%s: workspace of %lld bytes, %lld needed", who, (long long)plan_ws_bytes, (long long)v->total);
    if (misaligned(plan_ws)) return pg_fail(PG_EINVAL, several ? "%s: workspaces must be 256-byte aligned" : "%s: workspace must be 256-byte aligned", who);
    return PG_OK;
}

// the workspace as a count left it.  n_words_name: what the entry point calls the word count the plan was made for
int plan_view(const pg_table *t, int64_t n_words, const void *plan_ws, int64_t plan_ws_bytes, const char *who, const char *n_words_name, ConstPlanView *v)
{
    return plan_carve(t, n_words, plan_ws, plan_ws_bytes, v) ? PG_OK : pg_fail(PG_EINVAL, "%s: plan workspace does not match %s", who, n_words_name);
}

MiniView mini_view(const pg_table *t) { return MiniView{(uint64_t *)t->data, t->log2_slots, t->log2_bucket_slots, t->k}; }

// the SLOTS form of the lookups needs a row and a slot index in one 32-bit word (PG_MINI_PROBE_TWICE forces the general form)
// row groups that the count kernel's own scatter reaches in one pass: 2^11 (131 072 rows; 2048 digits in its lookup tiles)
constexpr int MINI_ONE_PASS_BITS = 11;
bool mini_slots_form(const pg_table *t, const pg_rows *rows)
{
    return rows && rows->n_rows > 0 && rows->n_rows < ((int64_t)1 << (32 - t->log2_bucket_slots)) - 1 && !getenv("PG_MINI_PROBE_TWICE");
}

// merged lookups (mini_count_kernel<..., MERGE>): the slot form, with room for the run length on top of row and bin.  The default
// wherever it applies and the caller gave pg_mini_count the word buffer it needs (PG_MINI_MERGE=0: the word-wise form): on
// config 2 the step is 0.3-2 ms shorter (box to box), the row histograms see 0.28 of the words
bool mini_merge_form(const pg_table *t, const pg_rows *rows, int vsize)
{
    const char *want = getenv("PG_MINI_MERGE");
    if ((want && atoi(want) == 0) || getenv("PG_MINI_NO_MERGE")) return false;
    if (!mini_slots_form(t, rows) || vsize < 1 || rows->n_rows >= ((int64_t)1 << 20)) return false;
    int vbits = 1, gbits = 0;
    while ((1 << vbits) < vsize) ++vbits;
    const int64_t n_groups = (rows->n_rows + 63) >> 6;
    while (((int64_t)1 << gbits) < n_groups) ++gbits;
    return vbits + 6 + gbits <= MERGE_CSHIFT;
}

// the record workspace: [bases A | bases B | meta A | meta B] of `cap` records each (8-byte bases, 4-byte meta words)
struct MiniRecLayout { size_t cap, bases_b_off, meta_a_off, meta_b_off, total; };
MiniRecLayout mini_rec_layout(size_t cap)
{
    return MiniRecLayout{cap, 8 * cap, 16 * cap, 20 * cap, 24 * cap};
}

// the largest record capacity (a multiple of 256) whose layout fits a workspace of that many bytes
size_t mini_rec_cap(int64_t rec_ws_bytes)
{
    size_t cap = 0;
    if (rec_ws_bytes > 0) {
        cap = (size_t)rec_ws_bytes / 24 / 256 * 256;
        while (cap >= 256 && mini_rec_layout(cap).total > (size_t)rec_ws_bytes) cap -= 256;
    }
    return cap;
}

template <bool CONST> struct RecViewT { size_t cap; ws_ptr<CONST, uint64_t> bases_a, bases_b; ws_ptr<CONST, uint32_t> meta_a, meta_b; };
using RecView = RecViewT<false>; using ConstRecView = RecViewT<true>;
template <bool CONST> int rec_view(ws_ptr<CONST, void> rec_ws, int64_t rec_ws_bytes, const char *who, RecViewT<CONST> *v)
{
    if (!CONST && misaligned(rec_ws)) return pg_fail(PG_EINVAL, "%s: workspaces must be 256-byte aligned", who);
    const MiniRecLayout l = mini_rec_layout(mini_rec_cap(rec_ws_bytes));
    if (l.cap < 256) return pg_fail(PG_EINVAL, "%s: record workspace of %lld bytes (pg_mini_records_bytes)", who, (long long)rec_ws_bytes);
    const auto ws = (ws_ptr<CONST, char>)rec_ws;
    v->cap = l.cap; v->bases_a = (ws_ptr<CONST, uint64_t>)ws; v->bases_b = (ws_ptr<CONST, uint64_t>)(ws + l.bases_b_off);
    v->meta_a = (ws_ptr<CONST, uint32_t>)(ws + l.meta_a_off); v->meta_b = (ws_ptr<CONST, uint32_t>)(ws + l.meta_b_off);
    return PG_OK;
}

// workspace of the count half (N > 1 ranks, see the kernels above): entry slabs | occupancy bitmaps | ring counts
struct MiniHalfLayout { size_t ent_off, occ_off, ring_off, total; };
MiniHalfLayout mini_half_layout(const pg_table *t)
{
    const size_t nb = (size_t)1 << (t->log2_slots - t->log2_bucket_slots), n_slots = (size_t)1 << t->log2_bucket_slots;
    const size_t n_occ = n_slots >= 64 ? n_slots / 64 : 1;
    MiniHalfLayout l;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
    l.ent_off = take(nb * n_slots * 8);
    l.occ_off = take(nb * n_occ * 8);
    l.ring_off = take(nb * 4);
    l.total = o;
    return l;
}

template <bool CONST> struct HalfViewT { ws_ptr<CONST, unsigned long long> ent, occ; ws_ptr<CONST, uint32_t> ring; };
using HalfView = HalfViewT<false>; using ConstHalfView = HalfViewT<true>;
template <bool CONST> int half_view(const pg_table *local, ws_ptr<CONST, void> half_ws, int64_t half_ws_bytes, const char *who, HalfViewT<CONST> *v)
{
    const MiniHalfLayout l = mini_half_layout(local);
    if (CONST && (int64_t)l.total > half_ws_bytes) return pg_fail(PG_EINVAL, "%s: workspace does not match the table", who);
    if (!CONST && ((int64_t)l.total > half_ws_bytes || misaligned(half_ws)))
        return pg_fail(PG_EINVAL, "%s: workspace of %lld bytes (256-byte aligned), %lld needed", who, (long long)half_ws_bytes, (long long)l.total);
    const auto ws = (ws_ptr<CONST, char>)half_ws;
    v->ent = (ws_ptr<CONST, unsigned long long>)(ws + l.ent_off); v->occ = (ws_ptr<CONST, unsigned long long>)(ws + l.occ_off);
    v->ring = (ws_ptr<CONST, uint32_t>)(ws + l.ring_off);
    return PG_OK;
}

int check_mini_rows(const pg_rows *rows, const char *who)
{
    if (!rows) return PG_OK;
    if (rows->n_rows < 0 || rows->n_rows > PG_MINI_MAX_ROWS) return pg_fail(PG_EINVAL, "%s: %lld rows (at most %d per launch)", who, (long long)rows->n_rows, PG_MINI_MAX_ROWS);
    if (rows->n_rows > 0 && (!rows->row_start || !rows->row_end)) return pg_fail(PG_EINVAL, "%s: null row arrays", who);
    return PG_OK;
}

// ---- typed dispatch (int_tag, with_flag, launch: pg_device.hpp); the helpers below list the cases of this file's kernels

// the first-pass kernels are instantiated per window length (registers of the rolling minimum); k > 21 runs the delayed
// central window of 8 or 9 M-mers (mini_window).  f(WindowTag<W, DELAY, M>, woff)
template <int W_, bool DELAY_, int M_> struct WindowTag { static constexpr int W = W_, M = M_; static constexpr bool DELAY = DELAY_; };
template <class F> int with_window(int k, F &&f)
{
    int wc, woff;
    mini_window(k, &wc, &woff);
    if (k > PG_HASH_MAX_K) return wc == 8 ? f(WindowTag<8, true, MINI_M>{}, woff) : f(WindowTag<9, true, MINI_M>{}, woff);
    if (mini_m(k) == MINI_M_SMALL)
        return wc == 3 ? f(WindowTag<3, false, MINI_M_SMALL>{}, woff) : wc == 4 ? f(WindowTag<4, false, MINI_M_SMALL>{}, woff) : f(WindowTag<5, false, MINI_M_SMALL>{}, woff);
    switch (wc) {
    case 4: return f(WindowTag<4, false, MINI_M>{}, woff);
    case 5: return f(WindowTag<5, false, MINI_M>{}, woff);
    case 6: return f(WindowTag<6, false, MINI_M>{}, woff);
    case 7: return f(WindowTag<7, false, MINI_M>{}, woff);
    case 8: return f(WindowTag<8, false, MINI_M>{}, woff);
    default: return f(WindowTag<9, false, MINI_M>{}, woff);
    }
}

// k-mers per record at most (as the first pass cuts them): f(int_tag<4 | 6 | 8 | 9>)
template <class F> int with_cap(int cap, F &&f)
{
    const int c = cap_class(cap);
    return c == 4 ? f(int_tag<4>{}) : c == 6 ? f(int_tag<6>{}) : c == 8 ? f(int_tag<8>{}) : f(int_tag<9>{});
}

// threads and row-group digits of a lookup workgroup (LookupLds / MergeLds): f(GeomTag<BLK, DIG>) for the three that exist
template <int BLK_, int DIG_> struct GeomTag { static constexpr int BLK = BLK_, DIG = DIG_; };
template <class F> auto with_lookup_geom(int blk, int dig, F &&f)
{
    return dig == 2048 ? f(GeomTag<BIG_BLOCK, 2048>{}) : blk == 512 ? f(GeomTag<512, 1024>{}) : f(GeomTag<BIG_BLOCK, 1024>{});
}

// (the kernel's SLOTS, WIDE, MERGE, HALF, MASKED; threads of a workgroup, row-group digits of its lookup tiles; dynamic LDS)
struct CountForm { bool slots, wide, merge, half, masked; int blk, dig; size_t lds; };
// slots / merge: mini_slots_form / mini_merge_form hold and the lookups are wanted; half: any of the count halves (N > 1 ranks, or a
// piece of a stream); gb1: first-pass digits of the row shuffle the lookups scatter into (0 where the launch does none)
CountForm count_form(const pg_table *t, const pg_rows *rows, bool slots, bool merge, bool half, bool masked, int gb1)
{
    CountForm f{slots, t->kind == PG_TABLE_MINI_WIDE, merge, half, masked, 0, 0, 0};
    const size_t table_lds = (size_t)(f.wide ? 12 : 8) << t->log2_bucket_slots;          // (wide: 8-byte keys + 4-byte counts per slot)
    // Buckets of at most 2^13 8-byte slots (64 KiB): 512-thread workgroups, TWO per CU -- one can be in its count loop (VALU, waits)
    // while the other is in its lookup phase (LDS throughput).  PG_COUNT_BLOCK=1024: the one-workgroup form for such tables too.
    const char *blk_env = getenv("PG_COUNT_BLOCK");
    const bool many_groups = slots && rows->n_rows > ((int64_t)1 << (PG_SHUFFLE_ONE_PASS_BITS + 6));     // more than 2^10 row groups: 2048 digits
    // (the count half does no lookups: the row-group digits do not matter to its geometry)
    const bool two_per_cu = !f.wide && slots && t->log2_bucket_slots <= 13 && (!many_groups || half) && !(blk_env && atoi(blk_env) == 1024);
    f.blk = two_per_cu ? 512 : BIG_BLOCK;
    f.dig = !half && !two_per_cu && gb1 > 10 ? 2048 : 1024;
    f.lds = table_lds + (size_t)(two_per_cu ? 512 / 64 : COUNT_WAVES) * RING * 12;      // table + the wavefronts' rings
    // the count kernel scatters its words into the row shuffle's group regions itself: its lookup phase (the table has become 2-byte bins by then) may need more
    if (slots && !half)
        f.lds = std::max(f.lds, with_lookup_geom(f.blk, f.dig, [&](auto g) { using G = decltype(g); return merge ? (size_t)MergeLds<G::BLK, G::DIG>::END : (size_t)LookupLds<G::BLK, G::DIG>::END; }));
    return f;
}

// calls f(kernel) if `c` is this instantiation
template <int CAP, bool SLOTS, bool WIDE, int BLK, int DIG, bool MERGE, bool HALF, bool MASKED, class F>
bool count_form_is(const CountForm &c, F &f, int *rc)
{
    if (c.slots != SLOTS || c.wide != WIDE || c.blk != BLK || c.dig != DIG || c.merge != MERGE || c.half != HALF || c.masked != MASKED) return false;
    *rc = f(mini_count_kernel<CAP, SLOTS, WIDE, BLK, DIG, MERGE, HALF, MASKED>);
    return true;
}

// every mini_count_kernel there is (for each of the four caps): f(kernel) for the one that `c` names
template <int CAP, class F> int with_count_kernel(const CountForm &c, F f)
{
    int rc = PG_OK;
    const bool found =
        //                 SLOTS  WIDE   BLK   DIG   MERGE  HALF   MASKED
        // the general form (no lookups, or a row and a slot index do not fit one word): packed and wide tables
        count_form_is<CAP, false, false, 1024, 1024, false, false, false>(c, f, &rc) ||
        count_form_is<CAP, false, true,  1024, 1024, false, false, false>(c, f, &rc) ||
        // one GPU, the slot form: word-wise or merged lookups; one workgroup per CU (1024 or, past 2^16 rows, 2048 digits) ...
        count_form_is<CAP, true,  false, 1024, 1024, false, false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 1024, 1024, true,  false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 1024, 2048, false, false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 1024, 2048, true,  false, false>(c, f, &rc) ||
        // ... or two per CU (buckets of at most 2^13 slots)
        count_form_is<CAP, true,  false, 512,  1024, false, false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 512,  1024, true,  false, false>(c, f, &rc) ||
        // the same on wide tables (one workgroup per CU only)
        count_form_is<CAP, true,  true,  1024, 1024, false, false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  true,  1024, 1024, true,  false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  true,  1024, 2048, false, false, false>(c, f, &rc) ||
        count_form_is<CAP, true,  true,  1024, 2048, true,  false, false>(c, f, &rc) ||
        // the count half (N > 1 ranks, pieces): packed slots, no lookups of its own
        count_form_is<CAP, true,  false, 1024, 1024, false, true,  false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 1024, 1024, true,  true,  false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 512,  1024, false, true,  false>(c, f, &rc) ||
        count_form_is<CAP, true,  false, 512,  1024, true,  true,  false>(c, f, &rc) ||
        // the masked count half: merged only
        count_form_is<CAP, true,  false, 1024, 1024, true,  true,  true >(c, f, &rc) ||
        count_form_is<CAP, true,  false, 512,  1024, true,  true,  true >(c, f, &rc);
    // (not reached: count_form and the checks in front of it give one of the forms above)
    return found ? rc : pg_fail(PG_EINVAL, "pg_mini_count: no kernel of this form");
}

// threads and digits of the merged lookups that run as kernels of their own (a piece's, a count half's).  More than 2^10 row groups:
// 2048 digits.  n_rank (the lookup half of N > 1 ranks) on buckets of at most 2^13 slots (what a rank's own reads need at 4+ ranks):
// 512-thread workgroups, two per CU -- that kernel starts cold (bins, meta words and provisional slots all come from HBM, where
// the one-GPU kernel's lookup phase finds them in L2), and a second workgroup on the CU hides what one alone waits for:
// 7.8 -> 5.9 ms, rehearsed 8-rank step 34.3 -> 32.3 ms on one box (PG_LOOKUP_HALF_1024=1: the one-workgroup form)
struct LookupGeom { int blk, dig; };
LookupGeom merged_lookup_geom(const pg_table *t, int gb1, bool n_rank)
{
    return gb1 > 10 ? LookupGeom{BIG_BLOCK, 2048} : n_rank && t->log2_bucket_slots <= 13 && !getenv("PG_LOOKUP_HALF_1024") ? LookupGeom{512, 1024} : LookupGeom{BIG_BLOCK, 1024};
}

// ---- what the lookup entries share: the plan workspace as a count left it (n_words_plan words, which the entry point calls
// n_words_name) and the row shuffle's regions for n_words_shuffle words.  merge: the merged lookups (no input buffer in the
// shuffle's layout, counted 4-byte words); begun: pg_mini_lookup_begin has prepared offsets and cursors (the piece forms) -- a
// further launch into them
enum class Lookups { word_wise, merged };
enum class Regions { prepare, begun };
struct LookupPrep { ConstPlanView plan; pg_shuffle_ctx ctx; ShufArgs sh; const unsigned long long *n_short; unsigned nb; };
int lookup_prepare(const pg_table *t, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_plan, const char *n_words_name,
                   int64_t n_words_shuffle, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *stream, Lookups form, Regions regions, const char *who, LookupPrep *l)
{
    int rc = plan_view(t, n_words_plan, plan_ws, plan_ws_bytes, who, n_words_name, &l->plan);
    if (rc) return rc;
    if (!l->plan.bits2) return pg_fail(PG_EINVAL, "%s: needs more than 256 buckets", who);
    pg_shuffle_ctx &ctx = l->ctx;
    const bool merge = form == Lookups::merged;
    if ((rc = pg_internal_shuffle_prepare(n_words_shuffle * 32, rows, vsize, shuffle_ws, shuffle_ws_bytes, stream, &ctx, MINI_ONE_PASS_BITS, merge ? 1 : 0, regions == Regions::begun ? 1 : 0))) return rc;
    if (ctx.gb1 > MINI_ONE_PASS_BITS) return pg_fail(PG_EINVAL, "%s: %d first-pass digits of the row shuffle", who, ctx.gb1);
    l->sh = ShufArgs{ctx.goff, ctx.gcur1, ctx.words_out, ctx.gb1, ctx.gb2, ctx.dshift, merge ? 0 : ctx.narrow, ctx.words_cap};
    l->n_short = l->plan.n_short(t->k);
    l->nb = 1u << l->plan.bits;
    return PG_OK;
}

}  // namespace

// (compiled into the translation unit whose kernels the flags change: a library linked from a checked / stamped / variant
// mini.o says so whatever its file name is)
extern "C" uint32_t pg_build_flags(void)
{
    uint32_t f = 0;
#ifdef PG_CHECKED
    f |= PG_BUILD_CHECKED;
#endif
#ifdef PG_MINI_STAMPS
    f |= PG_BUILD_STAMPS;
#endif
#ifdef PG_VARIANT
    f |= PG_BUILD_VARIANT;
#endif
    return f;
}

extern "C" int64_t pg_mini_plan_bytes(int64_t n_words, const pg_table *t)
{
    if (n_words < 0) return pg_fail(PG_EINVAL, "negative word count");
    int rc = check_mini(t, "pg_mini_plan_bytes");
    if (rc) return rc;
    MiniPlan p;
    plan_mini(t, n_words, &p);
    return (int64_t)p.total;
}

extern "C" int64_t pg_mini_records_bytes(int64_t n_records, const pg_table *t)
{
    if (n_records < 0) return pg_fail(PG_EINVAL, "negative record count");
    int rc = check_mini(t, "pg_mini_records_bytes");
    if (rc) return rc;
    const size_t n = ((size_t)n_records + 255) / 256 * 256 + 256;
    return (int64_t)mini_rec_layout(n).total;
}

// where the second meta plane of a record workspace of rec_ws_bytes starts
extern "C" int64_t pg_mini_records_meta_offset(int64_t rec_ws_bytes, const pg_table *t)
{
    int rc = check_mini(t, "pg_mini_records_meta_offset");
    if (rc) return rc;
    const size_t cap = mini_rec_cap(rec_ws_bytes);
    if (cap < 256) return pg_fail(PG_EINVAL, "pg_mini_records_meta_offset: record workspace of %lld bytes (pg_mini_records_bytes)", (long long)rec_ws_bytes);
    return (int64_t)mini_rec_layout(cap).meta_b_off;
}

// the library's own rule for the merged lookups (mini_merge_form): 1 where they apply to n_rows rows of this geometry, else 0
extern "C" int pg_mini_merge_form_applies(const pg_table *t, int64_t n_rows, int vsize)
{
    int rc = check_mini(t, "pg_mini_merge_form_applies");
    if (rc) return rc;
    if (n_rows < 0) return pg_fail(PG_EINVAL, "pg_mini_merge_form_applies: negative row count");
    if (t->kind != PG_TABLE_MINI) return 0;                       // (the merged lookups work on packed slots)
    const pg_rows r{nullptr, nullptr, n_rows, nullptr};
    return mini_merge_form(t, &r, vsize) ? 1 : 0;
}

extern "C" int64_t pg_mini_shuffle_bytes(int64_t n_words, int64_t n_rows, int vsize)
{
    if (n_words < 0 || n_rows < 0) return pg_fail(PG_EINVAL, "negative size");
    // (enough for either form of the row shuffle: the count kernel scattering into up to 2^11 row groups itself, or the general form)
    pg_shuffle_layout sl, sl1;
    int rc = pg_internal_shuffle_layout(n_words * 32, n_rows, vsize, &sl);
    if (rc) return rc;
    if ((rc = pg_internal_shuffle_layout(n_words * 32, n_rows, vsize, &sl1, MINI_ONE_PASS_BITS))) return rc;
    return (int64_t)(sl.total > sl1.total ? sl.total : sl1.total);
}

// the same for a caller that brings the merged lookups' slot buffer (pg_mini_merge_words): where that form applies and the row
// groups take one scatter pass, the provisional-word buffer of the row shuffle is not part of the layout (half the bytes)
extern "C" int64_t pg_mini_shuffle_bytes_merged(int64_t n_words, int64_t n_rows, int vsize, const pg_table *t)
{
    int rc = check_mini(t, "pg_mini_shuffle_bytes_merged");
    if (rc) return rc;
    if (n_words < 0 || n_rows < 0) return pg_fail(PG_EINVAL, "negative size");
    pg_rows r{nullptr, nullptr, n_rows, nullptr};
    if (!mini_merge_form(t, &r, vsize)) return pg_mini_shuffle_bytes(n_words, n_rows, vsize);
    pg_shuffle_layout sl;
    if ((rc = pg_internal_shuffle_layout(n_words * 32, n_rows, vsize, &sl, MINI_ONE_PASS_BITS, 1))) return rc;
    return (int64_t)sl.total;
}

// tabv: the table plane of the masked form (pg_mini_plan_masked), NULL otherwise
static int mini_plan_impl(const uint64_t *codes, const uint32_t *valid, const uint32_t *tabv, int64_t word_begin, int64_t word_end, const pg_table *t,
                          const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *stream)
{
    if (!codes || !valid || !plan_ws) return pg_fail(PG_EINVAL, "pg_mini_plan: null argument");
    if (word_begin < 0 || word_end < word_begin) return pg_fail(PG_EINVAL, "pg_mini_plan: bad word range");
    int rc = check_mini(t, "pg_mini_plan");
    if (rc) return rc;
    if ((rc = check_mini_rows(rows, "pg_mini_plan"))) return rc;
    PlanView p;
    if ((rc = plan_view(t, word_end - word_begin, plan_ws, plan_ws_bytes, "pg_mini_plan", false, &p))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n_regions = 1 << p.bits1;
    // (everything in front of round_row, the header first)
    if (hipMemsetAsync(p.header, 0, (size_t)((char *)p.round_row - (char *)p.header), s) != hipSuccess) return pg_fail(PG_EHIP, "pg_mini_plan: memset failed");
    if (hipMemsetAsync(p.chunk_tab, 0, ((size_t)p.n_chunks << p.bits1) * 8, s) != hipSuccess) return pg_fail(PG_EHIP, "pg_mini_plan: memset failed");
    const bool with_rows = rows && rows->n_rows > 0;
    if (word_end > word_begin) {
        if (with_rows)
            hipLaunchKernelGGL(round_rows_kernel, dim3((unsigned)((p.n_rounds + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, rows->row_end, rows->n_rows,
                               word_begin, p.n_rounds, p.round_row);
        // one workgroup per chunk (the kernel's chunk loop only matters beyond 2^20 chunks): with 4096 workgroups of five or six
        // chunks each, eight to a CU, the second half of them started together and ended one chunk apart -- 2.51 against 2.26 ms
        const int grid = (int)(p.n_chunks < (1 << 20) ? p.n_chunks : (1 << 20));
        rc = with_flag(tabv != nullptr, [&](auto masked) {
            return with_window(t->k, [&](auto w, int woff) {
                using Win = decltype(w);
                return launch(mini_plan_kernel<Win::W, Win::DELAY, Win::M, decltype(masked)::value>, dim3(grid), dim3(BLOCK), 0, s, "pg_mini_plan",
                              codes, valid, word_begin, word_end, t->k, woff, p.bits, p.bits2, mini_cap(t->k),
                              with_rows ? rows->row_start : nullptr, with_rows ? rows->row_end : nullptr, with_rows ? rows->n_rows : (int64_t)0,
                              with_rows ? rows->strict_valid : nullptr, p.round_row, p.chunk_tab, p.n_chunks, p.chunk_stride, p.header + 2, tabv);
            });
        });
        if (rc) return rc;
    }
    // records per region -> where the regions start -> exact offset of every (chunk, region) run; total -> header[0]
    hipLaunchKernelGGL(digit_totals_kernel, dim3((unsigned)n_regions), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)p.chunk_tab, p.n_chunks, p.region_tot);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)p.region_tot, (int64_t)n_regions, p.region_off);
    hipLaunchKernelGGL(digit_scan_kernel, dim3((unsigned)n_regions), dim3(BIG_BLOCK), 0, s, p.chunk_tab, p.n_chunks, (const unsigned long long *)p.region_off,
                       0, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(mini_total_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long *)p.region_off, n_regions, p.header);
    return check_launch("pg_mini_plan");
}

extern "C" int pg_mini_plan(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                            const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *stream)
{
    return mini_plan_impl(codes, valid, nullptr, word_begin, word_end, t, rows, plan_ws, plan_ws_bytes, stream);
}

extern "C" int pg_mini_plan_masked(const uint64_t *codes, const uint32_t *valid, const uint32_t *table_valid, int64_t word_begin, int64_t word_end,
                                   const pg_table *t, const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *stream)
{
    return mini_plan_impl(codes, valid, table_valid, word_begin, word_end, t, rows, plan_ws, plan_ws_bytes, stream);
}

static thread_local hipEvent_t first_pass_event = nullptr;         // recorded by every pg_mini_count behind its first scatter pass

// makes `stream` wait for the first scatter pass of this thread's latest pg_mini_count: work enqueued on it afterwards (the next
// batch's plan) overlaps the memory-bound second pass instead of the VALU-bound first one
extern "C" int pg_mini_wait_first_pass(void *stream)
{
    if (!first_pass_event) return pg_fail(PG_EINVAL, "pg_mini_wait_first_pass: no count yet");
    if (hipStreamWaitEvent((hipStream_t)stream, first_pass_event, 0) != hipSuccess) return pg_fail(PG_EHIP, "pg_mini_wait_first_pass: wait failed");
    return PG_OK;
}

// what the count entry points hand to mini_count_impl.  tabv: the table plane of the masked form, NULL otherwise.
// `half` (N > 1 ranks): the count half only -- no slice, no lookups; the bucket workgroups leave entries, occupancy and what
// the lookup half needs (HalfArgs).  `t` is then the rank's LOCAL geometry (the union's buckets, slots for the rank's own
// k-mers); its slots are never written.  half->accum != 0: a piece (no lookups in this launch, no row shuffle)
struct CountArgs {
    const uint64_t *codes; const uint32_t *valid, *tabv; int64_t word_begin, word_end; const pg_table *t; const pg_rows *rows;
    void *plan_ws; int64_t plan_ws_bytes; void *rec_ws; int64_t rec_ws_bytes; int window, vsize;
    void *shuffle_ws; int64_t shuffle_ws_bytes; void *merge_ws; int64_t merge_ws_words; const HalfArgs *half; uint32_t *status; void *stream;
    bool find = false;                                          // pg_mini_find: the table is finished and only read (mini_find_kernel)
};

static int mini_count_impl(const CountArgs &a)
{
    const pg_table *t = a.t; const pg_rows *rows = a.rows;
    const int window = a.window, vsize = a.vsize;
    const int64_t n_words = a.word_end - a.word_begin;
    const char *who = a.find ? "pg_mini_find" : "pg_mini_count";
    // ---- every refusal comes before anything is enqueued
    if (!a.codes || !a.valid || !a.plan_ws || !a.rec_ws || !a.status) return pg_fail(PG_EINVAL, "%s: null argument", who);
    if (a.word_begin < 0 || a.word_end < a.word_begin) return pg_fail(PG_EINVAL, "%s: bad word range", who);
    int rc = check_mini(t, who);
    if (rc) return rc;
    if ((rc = check_mini_rows(rows, who))) return rc;
    const bool with_rows = rows && rows->n_rows > 0, some_words = n_words > 0;
    if (window < 0 || vsize < 0 || (window > 0) != (vsize > 0)) return pg_fail(PG_EINVAL, "%s: window %d / vector size %d", who, window, vsize);
    const bool half = a.half != nullptr, piece = half && a.half->accum;
    if (window > 0) {
        if (!with_rows) return pg_fail(PG_EINVAL, "%s: the lookup pass needs rows", who);
        if (!a.shuffle_ws && !piece) return pg_fail(PG_EINVAL, "%s: null shuffle workspace", who);
        if (vsize > PG_SHUFFLE_MAX_VSIZE || (t->kind == PG_TABLE_MINI && (int64_t)window * vsize > (int64_t)PG_HASH_COUNT_SAT))
            return pg_fail(PG_EINVAL, "%s: window %d x vector size %d outside the exact range of the table", who, window, vsize);
    }
    PlanView p;
    RecView rec;
    if ((rc = plan_view(t, n_words, a.plan_ws, a.plan_ws_bytes, who, true, &p))) return rc;
    if ((rc = rec_view(a.rec_ws, a.rec_ws_bytes, who, &rec))) return rc;
    const bool slots_form = window > 0 && mini_slots_form(t, rows);
    const bool merge = window > 0 && a.merge_ws && a.merge_ws_words > 0 && mini_merge_form(t, rows, vsize);
    pg_shuffle_layout sl{0, 0, 0, 0, 0};
    if (window > 0 && !piece) {
        if ((rc = pg_internal_shuffle_layout(n_words * 32, rows->n_rows, vsize, &sl, slots_form ? MINI_ONE_PASS_BITS : PG_SHUFFLE_ONE_PASS_BITS, merge ? 1 : 0))) return rc;
        if ((int64_t)sl.total > a.shuffle_ws_bytes || misaligned(a.shuffle_ws))
            return pg_fail(PG_EINVAL, "%s: shuffle workspace of %lld bytes (256-byte aligned), %lld needed", who, (long long)a.shuffle_ws_bytes, (long long)sl.total);
    }
    if (a.merge_ws && misaligned(a.merge_ws)) return pg_fail(PG_EINVAL, "%s: workspaces must be 256-byte aligned", who);
    if (half && (t->kind == PG_TABLE_MINI_WIDE || !slots_form))
        return pg_fail(PG_EINVAL, "pg_mini_count_half: needs packed slots (k <= %d), rows and fewer than 2^(32 - log2 bucket slots) of them", PG_HASH_MAX_K);
    if (half && !p.bits2) return pg_fail(PG_EINVAL, "pg_mini_count_half: needs more than 256 buckets");
    if (piece && !merge) return pg_fail(PG_EINVAL, "pg_mini_count_piece: needs the merged lookups (fewer than 2^20 rows, their slot buffer given)");
    if (a.tabv && !(half && merge && rows->n_rows <= PG_MINI_MASKED_MAX_ROWS))
        return pg_fail(PG_EINVAL, "pg_mini_count_half_masked: needs the merged lookups (their slot buffer given) and at most %d rows", PG_MINI_MASKED_MAX_ROWS);
    hipStream_t s = (hipStream_t)a.stream;
    const int nb = 1 << p.bits, cap_k = mini_cap(t->k);
    // ---- clear: hist | cur2 | cur2l | kwords (they lie in a row), and the word cursor
    if (hipMemsetAsync(p.hist, 0, (size_t)((char *)p.wbeg - (char *)p.hist), s) != hipSuccess || hipMemsetAsync(p.header + 1, 0, 8, s) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: memset failed", who);
    // ---- first pass: the stream -> records, sorted by region
    if (some_words) {
        rc = with_flag(a.tabv != nullptr, [&](auto masked) {
            return with_window(t->k, [&](auto w, int woff) {
                using Win = decltype(w);
                constexpr bool MASKED = decltype(masked)::value;
                const size_t lds1 = MASKED ? sizeof(Scatter1LdsMasked<256>) : sizeof(Scatter1Lds<256>);
                return launch(mini_scatter_kernel<Win::W, Win::DELAY, Win::M, 256, MASKED>, dim3((unsigned)p.n_chunks), dim3(S1_BLOCK), lds1, s, who,
                              a.codes, a.valid, a.word_begin, a.word_end, t->k, woff, p.bits, p.bits2, cap_k,
                              with_rows ? rows->row_start : nullptr, with_rows ? rows->row_end : nullptr, with_rows ? rows->n_rows : (int64_t)0,
                              with_rows ? rows->strict_valid : nullptr, p.round_row, rec.bases_a, rec.meta_a, p.chunk_tab, p.n_chunks, p.chunk_stride,
                              p.header, p.region_off, (unsigned long long)rec.cap, a.status, a.tabv);
            });
        });
        if (rc) return rc;
    }
    // (for pg_mini_wait_first_pass: what is enqueued on another stream behind this event runs beside the second pass and the count)
    if (!first_pass_event && hipEventCreateWithFlags(&first_pass_event, hipEventDisableTiming) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: event creation failed", who);
    if (hipEventRecord(first_pass_event, s) != hipSuccess) return pg_fail(PG_EHIP, "%s: event record failed", who);
    // ---- bucket offsets: records per bucket from the regions' meta plane -> where every bucket starts (an empty range: all zero)
    if (p.bits2) {
        const int tiles_h = 32;
        if (some_words)
            hipLaunchKernelGGL(mini_bucket_hist_kernel, dim3((unsigned)(tiles_h << p.bits1)), dim3(BLOCK), 0, s, (const uint32_t *)rec.meta_a,
                               (const unsigned long long *)p.region_off, p.bits2, tiles_h, p.hist, (const unsigned long long *)p.header, (unsigned long long)rec.cap, (const uint32_t *)a.status);
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(BIG_BLOCK), 0, s, (const unsigned long long *)p.hist, (int64_t)nb, p.off);
    }
    const unsigned long long *off = p.bits2 ? p.off : p.region_off;             // (at most 256 buckets: buckets = regions)
    // ---- second pass: every region -> its buckets, short records first
    if (some_words && p.bits2) {
        // 256 digits: about one workgroup per tile of a region (from the record capacity: the count itself is on the device); with
        // the regions' workgroups on one XCD each, 96 workgroups per region walking a dozen tiles each took 3.32 ms where 576 to 1152
        // take 3.05.  512 digits: one workgroup per CU fits, so 16 per region walk a dozen tiles each with the next one
        // prefetched (tiles of 512 x 16 records: 2.99 ms with 16 per region; 8: 3.30, 32 to 64: 2.99-3.01, 128: 3.12, one tile
        // per workgroup without the prefetch: 3.29.  512 x 20: 2.89-3.00, 512 x 24: 2.82-2.95)
        const bool dig512 = p.bits2 > 7;
        const size_t tile = dig512 ? (size_t)S2Geom<512, 512, 24>::TILE : (size_t)S2Geom<256, BLOCK, 16>::TILE;
        const int tiles_x = (int)std::min<size_t>(dig512 ? 16 : 2048, std::max<size_t>(8, rec.cap / (tile << p.bits1) + 1));
        auto second_pass = [&](auto dig, auto blk, auto rpl, auto prefetch) {
            constexpr int DIG = decltype(dig)::value, BLK = decltype(blk)::value, RPL = decltype(rpl)::value;
            // (the merged lookups size their buffer from record counts: the second pass need not tally the k-mers in rows per bucket)
            return launch(mini_scatter2_kernel<DIG, BLK, RPL, decltype(prefetch)::value>, dim3((unsigned)(tiles_x << p.bits1)), dim3(BLK),
                          sizeof(Scatter2Lds<DIG, BLK, RPL>), s, who, rec.bases_a, rec.meta_a, off, p.bits2, tiles_x,
                          cap_k > SHORT_MAX ? SHORT_MAX : 0, rec.bases_b, rec.meta_b, p.cur2, p.cur2l, merge ? nullptr : p.kwords, p.header,
                          (unsigned long long)rec.cap, a.status);
        };
        rc = dig512 ? second_pass(int_tag<512>{}, int_tag<512>{}, int_tag<24>{}, std::true_type{}) : second_pass(int_tag<256>{}, int_tag<BLOCK>{}, int_tag<16>{}, std::false_type{});
        if (rc) return rc;
    }
    // ---- count (and, but for the halves, the lookups): one workgroup per bucket
    const bool shuffles = window && !piece;
    char *shuffle_ws = (char *)a.shuffle_ws;
    uint32_t *words_e = shuffles ? (uint32_t *)(shuffle_ws + sl.words_e_off) : nullptr;
    uint32_t *words_a = shuffles ? (uint32_t *)(shuffle_ws + sl.words_a_off) : nullptr;
    unsigned long long *emit_end = shuffles ? (unsigned long long *)(shuffle_ws + sl.emit_off) : nullptr;
    ShufArgs sh{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0ull};
    if (slots_form && !piece) {
        // the count kernel scatters its words into the row shuffle's group regions itself: offsets and cursors must be ready
        pg_shuffle_ctx ctx;
        if ((rc = pg_internal_shuffle_prepare(n_words * 32, rows, vsize, a.shuffle_ws, a.shuffle_ws_bytes, a.stream, &ctx, MINI_ONE_PASS_BITS, merge ? 1 : 0))) return rc;
        sh = ShufArgs{ctx.goff, ctx.gcur1, ctx.words_out, ctx.gb1, ctx.gb2, ctx.dshift, merge ? 0 : ctx.narrow, ctx.words_cap};
        words_a = ctx.words_in;                          // the provisional words wait in the shuffle's input buffer
        if (sh.gb1 > MINI_ONE_PASS_BITS) return pg_fail(PG_EINVAL, "%s: %d first-pass digits of the row shuffle", who, sh.gb1);
    }
    const CountForm form = count_form(t, rows, slots_form, merge, half, a.tabv != nullptr, sh.gb1);
    const MergeArgs mg{(uint32_t *)a.merge_ws, (unsigned long long)(a.merge_ws ? a.merge_ws_words : 0)};
    HalfArgs hv = half ? *a.half : HalfArgs{nullptr, nullptr, nullptr, nullptr, 0, nullptr};
    hv.meta_w = a.tabv ? (p.bits2 ? rec.meta_b : rec.meta_a) : nullptr;    // (the plane the count kernel reads: the lookup half reads it again)
    if (a.find) {
        // the find form: the count's geometry (512 threads, two workgroups per CU, on buckets of at most 2^13 slots), the slots and
        // then the lookup stage in the same LDS
        rc = with_cap(cap_k, [&](auto cap_c) {
            return with_lookup_geom(form.blk, form.dig, [&](auto geom) {
                using G = decltype(geom);
                const size_t lds = std::max((size_t)8 << t->log2_bucket_slots, (size_t)MergeLds<G::BLK, G::DIG>::END);
                return launch(mini_find_kernel<decltype(cap_c)::value, G::BLK, G::DIG>, dim3(nb), dim3(G::BLK), lds, s, who,
                              p.bits2 ? rec.bases_b : rec.bases_a, p.bits2 ? rec.meta_b : rec.meta_a, off, p.n_short(t->k), mini_view(t), window, vsize,
                              sl.vbits, p.header + 1, sh, mg, (unsigned long long)rec.cap, a.status);
            });
        });
        return rc ? rc : check_launch(who);
    }
    rc = with_cap(cap_k, [&](auto cap_c) {
        return with_count_kernel<decltype(cap_c)::value>(form, [&](auto kernel) {
            return launch(kernel, dim3(nb), dim3(form.blk), form.lds, s, "pg_mini_count", p.bits2 ? rec.bases_b : rec.bases_a, p.bits2 ? rec.meta_b : rec.meta_a,
                          off, p.n_short(t->k), p.bits2 ? p.kwords : nullptr, mini_view(t), window, vsize, sl.vbits, words_e, words_a, p.header + 1, p.wbeg,
                          emit_end, sh, mg, (unsigned long long)rec.cap, a.status, hv);
        });
    });
    return rc ? rc : check_launch("pg_mini_count");
}

extern "C" int pg_mini_count(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                             const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                             int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                             uint32_t *status, void *stream)
{
    return mini_count_impl(CountArgs{codes, valid, nullptr, word_begin, word_end, t, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                                     shuffle_ws, shuffle_ws_bytes, merge_ws, merge_ws_words, nullptr, status, stream});
}

// ---- abundance rows against a finished table (mini_find_kernel).  The one statement of where that form applies:
extern "C" int pg_mini_find_applies(const pg_table *t, int64_t n_rows, int window, int vsize)
{
    int rc = check_mini(t, "pg_mini_find_applies");
    if (rc) return rc;
    if (n_rows < 0) return pg_fail(PG_EINVAL, "pg_mini_find_applies: negative row count");
    if (t->kind != PG_TABLE_MINI) return 0;                       // (packed slots: 13 <= k <= 21)
    if (window < 1 || vsize < 1 || vsize > PG_SHUFFLE_MAX_VSIZE || (int64_t)window * vsize > (int64_t)PG_HASH_COUNT_SAT) return 0;
    const pg_rows r{nullptr, nullptr, n_rows, nullptr};
    return mini_merge_form(t, &r, vsize) ? 1 : 0;
}

extern "C" int pg_mini_find(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                            const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                            int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                            uint32_t *status, void *stream)
{
    int rc = check_mini(t, "pg_mini_find");
    if (rc) return rc;
    if (t->kind != PG_TABLE_MINI) return pg_fail(PG_EINVAL, "pg_mini_find: packed mini tables (%d <= k <= %d)", PG_MINI_MIN_K, PG_HASH_MAX_K);
    if (!rows || rows->n_rows < 1) return pg_fail(PG_EINVAL, "pg_mini_find: needs rows");
    if (!shuffle_ws || !merge_ws || merge_ws_words <= 0) return pg_fail(PG_EINVAL, "pg_mini_find: needs the shuffle workspace and the slot buffer");
    if ((rc = check_mini_rows(rows, "pg_mini_find"))) return rc;
    if (pg_mini_find_applies(t, rows->n_rows, window, vsize) != 1)
        return pg_fail(PG_EINVAL, "pg_mini_find: does not apply to %lld rows, window %d, vector size %d (pg_mini_find_applies)", (long long)rows->n_rows, window, vsize);
    CountArgs a{codes, valid, nullptr, word_begin, word_end, t, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                shuffle_ws, shuffle_ws_bytes, merge_ws, merge_ws_words, nullptr, status, stream};
    a.find = true;
    return mini_count_impl(a);
}

// ---- a stream counted in pieces (one GPU; see HalfArgs / mini_lookup_slice_merge_kernel)
extern "C" int pg_mini_count_piece(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                                   const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                                   int window, int vsize, void *merge_ws, int64_t merge_ws_words, int first, uint32_t *status, void *stream)
{
    int rc = check_mini(t, "pg_mini_count_piece");
    if (rc) return rc;
    if (t->kind != PG_TABLE_MINI) return pg_fail(PG_EINVAL, "pg_mini_count_piece: packed mini tables (13 <= k <= %d)", PG_HASH_MAX_K);
    if (window < 1 || vsize < 1 || !merge_ws) return pg_fail(PG_EINVAL, "pg_mini_count_piece: needs the abundance parameters and the slot buffer");
    const HalfArgs hv{nullptr, nullptr, nullptr, nullptr, first ? 1 : 2};
    return mini_count_impl(CountArgs{codes, valid, nullptr, word_begin, word_end, t, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                                     nullptr, 0, merge_ws, merge_ws_words, &hv, status, stream});
}

// offsets and cursors of the row shuffle for the words of ALL pieces (n_words_total: the words of the whole stream); once, before the
// first pg_mini_lookup_piece
extern "C" int pg_mini_lookup_begin(const pg_table *t, const pg_rows *rows, int64_t n_words_total, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *stream)
{
    int rc = check_mini(t, "pg_mini_lookup_begin");
    if (rc) return rc;
    if (!rows || !shuffle_ws || (rc = check_mini_rows(rows, "pg_mini_lookup_begin"))) return rc ? rc : pg_fail(PG_EINVAL, "pg_mini_lookup_begin: null argument");
    if (!mini_merge_form(t, rows, vsize)) return pg_fail(PG_EINVAL, "pg_mini_lookup_begin: the merged lookups do not apply to these rows");
    pg_shuffle_ctx ctx;
    return pg_internal_shuffle_prepare(n_words_total * 32, rows, vsize, shuffle_ws, shuffle_ws_bytes, stream, &ctx, MINI_ONE_PASS_BITS, 1);
}

// the lookups of one piece: plan_ws = the piece's plan workspace as pg_mini_count_piece left it (n_words_piece words), meta = the
// kept meta words of its bucket-ordered records (the second meta plane of its record workspace, n_records of them), merge_ws its
// slot buffer; the words go to the row shuffle's regions behind those of the pieces before.  pg_mini_abundance_from_emitted (with
// n_words_total) then writes the rows.
extern "C" int pg_mini_lookup_piece(const pg_table *t, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_piece,
                                    const uint32_t *meta, int64_t n_words_total, int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes,
                                    const void *merge_ws, uint32_t *status, void *stream)
{
    const char *who = "pg_mini_lookup_piece";
    int rc = check_mini(t, who);
    if (rc) return rc;
    if (t->kind != PG_TABLE_MINI || !rows || !plan_ws || !meta || !shuffle_ws || !merge_ws || !status || window < 1 || vsize < 1)
        return pg_fail(PG_EINVAL, "pg_mini_lookup_piece: bad argument");
    if ((rc = check_mini_rows(rows, who))) return rc;
    if (!mini_merge_form(t, rows, vsize)) return pg_fail(PG_EINVAL, "pg_mini_lookup_piece: the merged lookups do not apply to these rows");
    LookupPrep l;
    if ((rc = lookup_prepare(t, rows, plan_ws, plan_ws_bytes, n_words_piece, "n_words_piece", n_words_total, vsize, shuffle_ws, shuffle_ws_bytes, stream, Lookups::merged, Regions::begun, who, &l))) return rc;
    const LookupGeom g = merged_lookup_geom(t, l.ctx.gb1, false);
    rc = with_cap(mini_cap(t->k), [&](auto cap_c) {
        auto go = [&](auto dig) {
            constexpr int CAP = decltype(cap_c)::value, DIG = decltype(dig)::value;
            return launch(mini_lookup_slice_merge_kernel<CAP, BIG_BLOCK, DIG>, dim3(l.nb), dim3(BIG_BLOCK), MergeLds<BIG_BLOCK, DIG>::END, (hipStream_t)stream, who,
                          l.plan.off, l.n_short, l.plan.wbeg, mini_view(t), window, vsize, l.ctx.vbits, (const uint32_t *)merge_ws, meta, l.sh, status);
        };
        return g.dig == 2048 ? go(int_tag<2048>{}) : go(int_tag<1024>{});      // (one workgroup per CU: the slots are warm in L2 here)
    });
    return rc ? rc : check_launch(who);
}

// dwords of the merged form's provisional buffer (pg_mini_count's merge_ws): a halfword per k-mer slot of every batch of 64
// records of either class, a step's slack.  n_records / n_long_records: the first and third 8-byte word of the plan workspace.
extern "C" int64_t pg_mini_merge_words(int64_t n_words, int64_t n_records, int64_t n_long_records, const pg_table *t)
{
    int rc = check_mini(t, "pg_mini_merge_words");
    if (rc) return rc;
    if (n_words < 0 || n_records < 0 || n_long_records < 0 || n_long_records > n_records) return pg_fail(PG_EINVAL, "pg_mini_merge_words: bad counts");
    const int64_t nb = (int64_t)1 << (t->log2_slots - t->log2_bucket_slots);
    const int cap_t = cap_class(mini_cap(t->k));                     // (the kernels' instantiations)
    MiniPlan p;
    plan_mini(t, n_words, &p);
    const bool two = cap_t > SHORT_MAX && p.bits2 > 0;               // (without a second scatter pass the classes are not sorted apart: all "long")
    const int64_t n_long = two ? n_long_records : n_records, n_short = two ? n_records - n_long_records : 0;
    // (dwords: a batch of 64 records has a row of 64 halfwords = 32 dwords per k-mer of its class's cap; every bucket rounds both
    // classes up to whole batches; a step's slack behind the last bucket)
    const int64_t fixed = 32 * (int64_t)(two ? SHORT_MAX : cap_t) * (n_short / 64 + nb) + 32 * (int64_t)cap_t * (n_long / 64 + nb);
    return (fixed + 32 * 16 + 255) / 256 * 256;
}

// ---- N > 1 ranks (see the kernels above)
extern "C" int64_t pg_mini_half_bytes(const pg_table *local)
{
    int rc = check_mini(local, "pg_mini_half_bytes");
    if (rc) return rc;
    return (int64_t)mini_half_layout(local).total;
}

// accum: see HalfArgs (0: one launch; else a piece, for `who` = pg_mini_count_half_piece)
static int mini_count_half_impl(CountArgs a, void *half_ws, int64_t half_ws_bytes, int64_t *fill, int accum, const char *who)
{
    int rc = check_mini(a.t, who);
    if (rc) return rc;
    if (!half_ws || !fill) return pg_fail(PG_EINVAL, "%s: null argument", who);
    HalfView h;
    if ((rc = half_view(a.t, half_ws, half_ws_bytes, who, &h))) return rc;
    const HalfArgs hv{h.ent, h.occ, (long long *)fill, h.ring, accum, nullptr};
    a.half = &hv;
    return mini_count_impl(a);
}

extern "C" int pg_mini_count_half(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *local,
                                  const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                                  int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                                  void *half_ws, int64_t half_ws_bytes, int64_t *fill, uint32_t *status, void *stream)
{
    return mini_count_half_impl(CountArgs{codes, valid, nullptr, word_begin, word_end, local, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                                          shuffle_ws, shuffle_ws_bytes, merge_ws, merge_ws_words, nullptr, status, stream}, half_ws, half_ws_bytes, fill, 0, "pg_mini_count_half");
}

extern "C" int pg_mini_count_half_masked(const uint64_t *codes, const uint32_t *valid, const uint32_t *table_valid, int64_t word_begin, int64_t word_end,
                                         const pg_table *local, const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                                         int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                                         void *half_ws, int64_t half_ws_bytes, int64_t *fill, uint32_t *status, void *stream)
{
    return mini_count_half_impl(CountArgs{codes, valid, table_valid, word_begin, word_end, local, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                                          shuffle_ws, shuffle_ws_bytes, merge_ws, merge_ws_words, nullptr, status, stream}, half_ws, half_ws_bytes, fill, 0, "pg_mini_count_half");
}

extern "C" int pg_mini_gather_entries(const pg_table *local, const void *half_ws, int64_t half_ws_bytes, const int64_t *fill,
                                      const int64_t *dst_elem, uint64_t *out, int64_t out_elems, uint32_t *status, void *stream)
{
    int rc = check_mini(local, "pg_mini_gather_entries");
    if (rc) return rc;
    if (!half_ws || !fill || !dst_elem || !out || !status || out_elems < 0) return pg_fail(PG_EINVAL, "pg_mini_gather_entries: null argument");
    ConstHalfView h;
    if ((rc = half_view(local, half_ws, half_ws_bytes, "pg_mini_gather_entries", &h))) return rc;
    const unsigned nb = 1u << (local->log2_slots - local->log2_bucket_slots);
    hipLaunchKernelGGL(mini_gather_entries_kernel, dim3(nb), dim3(BLOCK), 0, (hipStream_t)stream, h.ent, local->log2_bucket_slots, (const long long *)fill,
                       (const long long *)dst_elem, (unsigned long long *)out, (unsigned long long)out_elems, status);
    return check_launch("pg_mini_gather_entries");
}

static int mini_merge_bins_impl(bool masked, const uint64_t *recv, int64_t part_stride, const int64_t *seg, int n_parts, const pg_table *t,
                                int64_t bucket_begin, int64_t bucket_end, int window, int vsize, uint16_t *bins_out, uint32_t *status, void *stream)
{
    int rc = check_mini(t, "pg_mini_merge_bins");
    if (rc) return rc;
    if (t->kind != PG_TABLE_MINI) return pg_fail(PG_EINVAL, "pg_mini_merge_bins: packed mini tables only");
    const int64_t nb = (int64_t)1 << (t->log2_slots - t->log2_bucket_slots);
    if (!recv || !seg || !bins_out || !status || n_parts < 1 || bucket_begin < 0 || bucket_end < bucket_begin || bucket_end > nb || window < 1 || vsize < 1)
        return pg_fail(PG_EINVAL, "pg_mini_merge_bins: bad arguments");
    if (bucket_end == bucket_begin) return PG_OK;
    rc = with_flag(masked, [&](auto m) {
        return launch(mini_merge_bins_kernel<decltype(m)::value>, dim3((unsigned)(bucket_end - bucket_begin)), dim3(BIG_BLOCK), (size_t)8 << t->log2_bucket_slots,
                      (hipStream_t)stream, "pg_mini_merge_bins", (const unsigned long long *)recv, part_stride, (const long long *)seg, n_parts,
                      (int)(bucket_end - bucket_begin), mini_view(t), bucket_begin, window, vsize, bins_out, status);
    });
    return rc ? rc : check_launch("pg_mini_merge_bins");
}

extern "C" int pg_mini_merge_bins(const uint64_t *recv, int64_t part_stride, const int64_t *seg, int n_parts, const pg_table *t,
                                  int64_t bucket_begin, int64_t bucket_end, int window, int vsize, uint16_t *bins_out, uint32_t *status, void *stream)
{
    return mini_merge_bins_impl(false, recv, part_stride, seg, n_parts, t, bucket_begin, bucket_end, window, vsize, bins_out, status, stream);
}

extern "C" int pg_mini_merge_bins_masked(const uint64_t *recv, int64_t part_stride, const int64_t *seg, int n_parts, const pg_table *t,
                                         int64_t bucket_begin, int64_t bucket_end, int window, int vsize, uint16_t *bins_out, uint32_t *status, void *stream)
{
    return mini_merge_bins_impl(true, recv, part_stride, seg, n_parts, t, bucket_begin, bucket_end, window, vsize, bins_out, status, stream);
}

extern "C" int pg_mini_lookup_half(const pg_table *local, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, const void *rec_ws, int64_t rec_ws_bytes,
                                   int64_t n_words_counted,
                                   int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, const void *merge_ws, int64_t merge_ws_words,
                                   const void *half_ws, int64_t half_ws_bytes,
                                   const uint16_t *bins_in, const int64_t *bin_elem, uint32_t *status, void *stream)
{
    const char *who = "pg_mini_lookup_half";
    int rc = check_mini(local, who);
    if (rc) return rc;
    if (!rows || !plan_ws || !shuffle_ws || !half_ws || !bins_in || !bin_elem || !status) return pg_fail(PG_EINVAL, "pg_mini_lookup_half: null argument");
    if ((rc = check_mini_rows(rows, who))) return rc;
    if (local->kind != PG_TABLE_MINI || !mini_slots_form(local, rows)) return pg_fail(PG_EINVAL, "pg_mini_lookup_half: not the slot form");
    ConstHalfView h;
    if ((rc = half_view(local, half_ws, half_ws_bytes, who, &h))) return rc;
    const bool merge = merge_ws && merge_ws_words > 0 && mini_merge_form(local, rows, vsize);         // (as the count half decided)
    ConstRecView rec{};
    if (merge) {
        // (the merged form reads the records' meta words again: lengths and rows say which provisional slots mean anything)
        if (!rec_ws) return pg_fail(PG_EINVAL, "pg_mini_lookup_half: the merged form needs the count half's record workspace");
        if ((rc = rec_view(rec_ws, rec_ws_bytes, who, &rec))) return rc;
    }
    // the row shuffle's regions: offsets and cursors as the count half's launch prepared them (same layout call)
    LookupPrep l;
    if ((rc = lookup_prepare(local, rows, plan_ws, plan_ws_bytes, n_words_counted, "n_words_counted", n_words_counted, vsize, shuffle_ws, shuffle_ws_bytes, stream, merge ? Lookups::merged : Lookups::word_wise, Regions::prepare, who, &l))) return rc;
    if (merge) {
        const LookupGeom g = merged_lookup_geom(local, l.ctx.gb1, true);
        rc = with_cap(mini_cap(local->k), [&](auto cap_c) {
            return with_lookup_geom(g.blk, g.dig, [&](auto geom) {
                using G = decltype(geom);
                return launch(mini_lookup_half_merge_kernel<decltype(cap_c)::value, G::BLK, G::DIG>, dim3(l.nb), dim3(G::BLK), MergeLds<G::BLK, G::DIG>::END, (hipStream_t)stream, who,
                              l.plan.off, l.n_short, l.plan.wbeg, h.ring, h.occ, bins_in, (const long long *)bin_elem, local->log2_bucket_slots, l.ctx.vbits,
                              (const uint32_t *)merge_ws, rec.meta_b, l.sh, status);
            });
        });
    } else {
        // 1024-thread workgroups whatever the bucket size: tiles of 16 Ki words keep the runs per row group at 32 bytes -- with
        // 512 threads (8 Ki-word tiles, two workgroups per CU) this kernel took 14.1 ms where the one-GPU kernel's lookup phase
        // takes 8.5 (PG_LOOKUP_HALF_512=1: that form, for comparison)
        const bool half_block = local->log2_bucket_slots <= 13 && l.ctx.gb1 <= 10 && getenv("PG_LOOKUP_HALF_512");
        rc = with_lookup_geom(half_block ? 512 : BIG_BLOCK, l.ctx.gb1 > 10 ? 2048 : 1024, [&](auto geom) {
            using G = decltype(geom);
            return launch(mini_lookup_half_kernel<G::BLK, G::DIG>, dim3(l.nb), dim3(G::BLK), LookupLds<G::BLK, G::DIG>::END, (hipStream_t)stream, who, l.plan.kwords, l.plan.wbeg, h.occ,
                          bins_in, (const long long *)bin_elem, local->log2_bucket_slots, l.ctx.vbits, l.ctx.words_in, l.sh, status);
        });
    }
    return rc ? rc : check_launch(who);
}

// ---- the count half in pieces (N > 1 ranks; see HalfArgs): `local` has real slots here (2^log2_slots words), which the pieces
// count into; the last piece leaves entries, occupancy and fill in half_ws as one pg_mini_count_half would
static int mini_count_half_piece_impl(CountArgs a, void *half_ws, int64_t half_ws_bytes, int64_t *fill, int first, int last)
{
    int rc = check_mini(a.t, "pg_mini_count_half_piece");
    if (rc) return rc;
    if (a.t->kind != PG_TABLE_MINI) return pg_fail(PG_EINVAL, "pg_mini_count_half_piece: packed mini tables (13 <= k <= %d)", PG_HASH_MAX_K);
    if (a.window < 1 || a.vsize < 1 || !a.merge_ws || a.merge_ws_words <= 0) return pg_fail(PG_EINVAL, "pg_mini_count_half_piece: needs the abundance parameters and the slot buffer");
    return mini_count_half_impl(a, half_ws, half_ws_bytes, fill, first ? (last ? 4 : 1) : (last ? 3 : 2), "pg_mini_count_half_piece");
}

extern "C" int pg_mini_count_half_piece(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *local,
                                        const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                                        int window, int vsize, void *merge_ws, int64_t merge_ws_words, void *half_ws, int64_t half_ws_bytes,
                                        int64_t *fill, int first, int last, uint32_t *status, void *stream)
{
    return mini_count_half_piece_impl(CountArgs{codes, valid, nullptr, word_begin, word_end, local, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                                                nullptr, 0, merge_ws, merge_ws_words, nullptr, status, stream}, half_ws, half_ws_bytes, fill, first, last);
}

extern "C" int pg_mini_count_half_piece_masked(const uint64_t *codes, const uint32_t *valid, const uint32_t *table_valid, int64_t word_begin, int64_t word_end,
                                               const pg_table *local, const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                                               int window, int vsize, void *merge_ws, int64_t merge_ws_words, void *half_ws, int64_t half_ws_bytes,
                                               int64_t *fill, int first, int last, uint32_t *status, void *stream)
{
    return mini_count_half_piece_impl(CountArgs{codes, valid, table_valid, word_begin, word_end, local, rows, plan_ws, plan_ws_bytes, rec_ws, rec_ws_bytes, window, vsize,
                                                nullptr, 0, merge_ws, merge_ws_words, nullptr, status, stream}, half_ws, half_ws_bytes, fill, first, last);
}

// the lookups of one piece of a count half in pieces, once the bins are back: plan_ws / meta / merge_ws of that piece (as for
// pg_mini_lookup_piece), half_ws / bins_in / bin_elem as for pg_mini_lookup_half; the row shuffle's regions of the whole stream
// were prepared by pg_mini_lookup_begin(local, rows, n_words_total, ...)
extern "C" int pg_mini_lookup_half_piece(const pg_table *local, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_piece,
                                         const uint32_t *meta, int64_t n_words_total, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes,
                                         const void *merge_ws, const void *half_ws, int64_t half_ws_bytes,
                                         const uint16_t *bins_in, const int64_t *bin_elem, uint32_t *status, void *stream)
{
    const char *who = "pg_mini_lookup_half_piece";
    int rc = check_mini(local, who);
    if (rc) return rc;
    if (local->kind != PG_TABLE_MINI || !rows || !plan_ws || !meta || !shuffle_ws || !merge_ws || !half_ws || !bins_in || !bin_elem || !status || vsize < 1)
        return pg_fail(PG_EINVAL, "pg_mini_lookup_half_piece: bad argument");
    if ((rc = check_mini_rows(rows, who))) return rc;
    if (!mini_merge_form(local, rows, vsize)) return pg_fail(PG_EINVAL, "pg_mini_lookup_half_piece: the merged lookups do not apply to these rows");
    ConstHalfView h;
    if ((rc = half_view(local, half_ws, half_ws_bytes, who, &h))) return rc;
    LookupPrep l;
    if ((rc = lookup_prepare(local, rows, plan_ws, plan_ws_bytes, n_words_piece, "n_words_piece", n_words_total, vsize, shuffle_ws, shuffle_ws_bytes, stream, Lookups::merged, Regions::begun, who, &l))) return rc;
    const LookupGeom g = merged_lookup_geom(local, l.ctx.gb1, true);
    rc = with_cap(mini_cap(local->k), [&](auto cap_c) {
        return with_lookup_geom(g.blk, g.dig, [&](auto geom) {
            using G = decltype(geom);
            return launch(mini_lookup_half_merge_kernel<decltype(cap_c)::value, G::BLK, G::DIG, true>, dim3(l.nb), dim3(G::BLK), MergeLds<G::BLK, G::DIG>::END,
                          (hipStream_t)stream, who, l.plan.off, l.n_short, l.plan.wbeg, h.ring, h.occ, bins_in, (const long long *)bin_elem,
                          local->log2_bucket_slots, l.ctx.vbits, (const uint32_t *)merge_ws, meta, l.sh, status);
        });
    });
    return rc ? rc : check_launch(who);
}

extern "C" int pg_mini_abundance_from_emitted(const pg_table *t, const pg_rows *rows, int vsize, int32_t *abd_out,
                                              const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_counted,
                                              void *shuffle_ws, int64_t shuffle_ws_bytes, void *stream)
{
    int rc = check_mini(t, "pg_mini_abundance_from_emitted");
    if (rc) return rc;
    if (!rows || !abd_out || !plan_ws || !shuffle_ws) return pg_fail(PG_EINVAL, "pg_mini_abundance_from_emitted: null argument");
    if ((rc = check_mini_rows(rows, "pg_mini_abundance_from_emitted"))) return rc;
    ConstPlanView p;
    if ((rc = plan_view(t, n_words_counted, plan_ws, plan_ws_bytes, "pg_mini_abundance_from_emitted", "n_words_counted", &p))) return rc;
    if (misaligned(shuffle_ws)) return pg_fail(PG_EINVAL, "pg_mini_abundance_from_emitted: workspace must be 256-byte aligned");
    if (mini_slots_form(t, rows))        // the count kernel has scattered the words by row group already
        return pg_internal_shuffle_finish(n_words_counted * 32, rows, vsize, abd_out, shuffle_ws, shuffle_ws_bytes, stream,
                                          mini_merge_form(t, rows, vsize) ? PG_SHUFFLE_WORDS_COUNTED
                                          : pg_internal_shuffle_is_narrow(n_words_counted * 32, rows->n_rows, vsize, MINI_ONE_PASS_BITS) ? PG_SHUFFLE_WORDS_NARROW
                                          : PG_SHUFFLE_WORDS_PLAIN, MINI_ONE_PASS_BITS, mini_merge_form(t, rows, vsize) ? 1 : 0);
    return pg_internal_shuffle_rows(p.wbeg, 1 << p.bits, n_words_counted * 32, rows, vsize, abd_out, shuffle_ws, shuffle_ws_bytes, stream);
}
