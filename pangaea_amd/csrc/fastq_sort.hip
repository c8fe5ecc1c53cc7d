// fastq_sort.hip -- the barcode of a read pair, on the FASTQ TEXT in device memory: where the BX:Z: tag of a header lies, 8-byte
// key words of the tags for a radix sort, and the full comparison of neighbouring tags (pangaea_amd/sortreads.py: sort_fastq,
// check_fastq).  Stands beside step 0 of the reference's driver, src/run_pangaea:237-252 (awk's match of /BX:Z:[^[:space:]]+/
// on the first header of an 8-line block, `LANG=C sort -k1,1`); semantics: the header's section "Read pairs of a FASTQ text by
// their barcode tag".  A translation unit of its own, so that work on it cannot touch the timed kernels' code objects.  The
// line index is pg_fastq_index's and the records are moved by pg_fastq_gather (table_ops.hip): nothing of that is repeated here.
//
// Shapes, and why:
//   tags     one wavefront per header, 64 bytes per turn, one byte per lane.  Everything the scan decides with is a ballot -- a
//            64-bit mask that is the same in every lane, so it lives in scalar registers and the control flow is scalar branches:
//            "is white space", and one mask per letter of the prefix.  "The five bytes BX:Z: END at position i" is the AND of
//            the five letter masks, each shifted to i; what a shift pushes beyond bit 63 belongs to the next turn, so the
//            previous turn's masks are kept (five scalar pairs) and shifted in from below: a prefix or a tag body that straddles
//            a turn boundary needs no second look at the bytes.  One more shift and `& ~space` gives the positions where a tag
//            BODY begins; the leftmost match is ctz of the first non-zero mask, its end the first white-space bit behind it.
//            A header of a 10x / stLFR read is 40 to 100 bytes -- one or two turns.  Per unit the wavefront makes two dependent
//            round trips to memory (its line starts; then the header's first turn together with the '@' / '+' bytes of its
//            records), and that chain, not bandwidth, is what the kernel's time is made of: 0.38 ms for 1 M headers, where one
//            trip per question took 0.54.  One lane per header would keep 64 units' loads in flight per wavefront, at the
//            price of a per-lane byte scan with state in vector registers and a loop that diverges with the header lengths;
//            not built, the stage being a thousandth of the call.  Measured numbers: DESIGN.md, "Sorting reads by barcode".
//   keys     one lane per unit: 8 bytes of the tag from byte_begin on, big-endian, zero behind the tag's end.
//   compare  one lane per neighbouring pair: memcmp in 8-byte steps, then the lengths; never looks at a key.
// The text and the arrays are read with plain loads and written with plain stores; the two status words of the tags kernel
// are updated as pg_table_read_hits updates them (atomicOr / atomicMin, on a malformed record only).  Whatever line_start,
// tag_off, tag_len and order hold, no byte outside [0, n_bytes) of the text is read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pangaea_feat.h"
#include "pg_internal.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int PREFIX = 5;                                    // strlen("BX:Z:")
constexpr int MAX_BODY = PG_FASTQ_MAX_TAG;
constexpr int64_t MAX_UNITS = 1LL << 40;

int grid_for(int64_t items, int per_block)
{
    int64_t blocks = (items + per_block - 1) / per_block;
    const int64_t cap = 256 * 16;                            // 256 CUs x 16 resident workgroups' worth, grid-stride beyond
    if (blocks > cap) blocks = cap;
    return blocks < 1 ? 1 : (int)blocks;
}

int check_launch(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return pg_fail(PG_EHIP, "%s: %s", what, hipGetErrorString(e));
    return PG_OK;
}

// C-locale white space: space and \t \n \v \f \r (9 .. 13)
__device__ __forceinline__ bool is_space(uint32_t c) { return c == ' ' || c - 9u <= 4u; }

// m << k, with the top k bits of the previous turn's mask coming in from below (0 < k < 64)
__device__ __forceinline__ uint64_t shift_in(uint64_t m, uint64_t prev, int k) { return (m << k) | (prev >> (64 - k)); }

// a tag that may be looked at: inside the text and no longer than the tags kernel writes one
__device__ __forceinline__ bool tag_ok(int64_t off, int32_t len, int64_t n_bytes)
{
    return off >= 0 && len > PREFIX && len <= PREFIX + MAX_BODY && off <= n_bytes - len;
}

// a 64-bit value of lane k, the same in every lane, in scalar registers
__device__ __forceinline__ int64_t from_lane(int64_t v, int k)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, k), hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), k);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// Per unit the wavefront makes TWO round trips to memory, not one per question: (1) the unit's 5 or 9 line starts, one per
// lane; (2) together, the first 64 bytes of the header and the '@' / '+' bytes of the unit's records (lane 2r: line 4r, lane
// 2r + 1: line 4r + 2).  Headers of more than 64 bytes take one more trip per turn.  What is asked of a record is what
// fastq_record_check of table_ops.hip asks, without the quality rule.
__global__ __launch_bounds__(BLOCK) void barcode_tags_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ line_start,
                                                             int64_t n_units, int lines_per_unit, long long *__restrict__ tag_off,
                                                             int32_t *__restrict__ tag_len, unsigned long long *status)
{
    const int lane = threadIdx.x & 63;
    // (the wavefront's number in a form the compiler knows to be the same in every lane: what follows from it stays scalar)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    const int records = lines_per_unit >> 2;
    for (int64_t u = (int64_t)blockIdx.x * WAVES + wave; u < n_units; u += n_waves) {
        const int64_t mine = lane <= lines_per_unit ? line_start[u * lines_per_unit + lane] : 0;
        const int64_t next = __shfl_down(mine, 1);
        // line k of a record begins in front of line k + 1 (its last line may be empty: the text's end), inside [0, n_bytes]
        const bool in_order = (lane & 3) == 3 ? mine <= next : mine < next;
        const uint64_t off_index = __ballot((lane < lines_per_unit && !in_order) || (lane == 0 && mine < 0) || (lane == lines_per_unit && mine > n_bytes));
        uint32_t bad = 0;
        int64_t bad_record = u * records;
        int64_t body = -1, end = -1;                         // first byte of the tag's body, first byte behind it
        if (off_index) {                                     // (no index of this text: nothing of the text is read)
            const int r = __builtin_ctzll(off_index) >> 2;
            bad = PG_FASTQ_BAD_INDEX;
            bad_record += r < records ? r : records - 1;
        } else {
            const int64_t a = from_lane(mine, 0), limit = from_lane(mine, 1);        // the header with its line end: 0 <= a < limit <= n_bytes
            const int64_t marker_at = __shfl(mine, (2 * lane) & 63);                 // lanes 0 .. 2 * records - 1: lines 0, 2, 4, 6 (all below n_bytes)
            const uint32_t marker = lane < 2 * records ? text[marker_at] : 0;
            uint32_t c = a + lane < limit ? text[a + lane] : ' ';    // (behind the line: white space, which ends a tag and begins none)
            const uint64_t off_marker = __ballot(lane < 2 * records && marker != ((lane & 1) ? '+' : '@'));
            if (off_marker) {
                const int m = __builtin_ctzll(off_marker);   // (record by record, '@' before '+': the order of fastq_record_check)
                bad = (m & 1) ? PG_FASTQ_NO_PLUS : PG_FASTQ_NO_AT;
                bad_record += m >> 1;
            } else {
                uint64_t pb = 0, px = 0, pc = 0, pz = 0, pe = 0;     // the previous turn's masks: 'B', 'X', ':', 'Z', "a prefix ends here"
                for (int64_t p0 = a;;) {
                    const uint64_t ws = __ballot(is_space(c));
                    if (body >= 0) {                         // inside the tag: its end is the first white space
                        if (ws) { end = p0 + __builtin_ctzll(ws); break; }
                    } else {
                        const uint64_t mb = __ballot(c == 'B'), mx = __ballot(c == 'X'), mc = __ballot(c == ':'), mz = __ballot(c == 'Z');
                        const uint64_t e = shift_in(mb, pb, 4) & shift_in(mx, px, 3) & shift_in(mc, pc, 2) & shift_in(mz, pz, 1) & mc;
                        const uint64_t f = shift_in(e, pe, 1) & ~ws;         // a prefix ends right in front and this byte is no white space
                        pb = mb; px = mx; pc = mc; pz = mz; pe = e;
                        if (f) {
                            const int b = __builtin_ctzll(f);                // the leftmost match
                            body = p0 + b;
                            const uint64_t rest = ws & ~((2ull << b) - 1);   // (b = 63: 2 << 63 is 0, the mask is empty)
                            if (rest) { end = p0 + __builtin_ctzll(rest); break; }
                        }
                    }
                    p0 += 64;
                    if (p0 >= limit) break;
                    c = p0 + lane < limit ? text[p0 + lane] : ' ';
                }
                if (body >= 0 && end < 0) end = limit;       // (a last line without newline)
                if (body >= 0 && end - body > MAX_BODY) bad = PG_FASTQ_LONG_TAG;
            }
        }
        if (lane == 0) {
            if (bad) {
                atomicMin(&status[1], ((unsigned long long)bad_record << 8) | bad);
                atomicOr(&status[0], (unsigned long long)PG_STATUS_FASTQ_FORMAT);
            }
            const bool tagged = !bad && body >= 0;
            tag_off[u] = tagged ? body - PREFIX : -1;
            tag_len[u] = tagged ? (int32_t)(end - body) + PREFIX : 0;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void tag_keys_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ tag_off,
                                                         const int32_t *__restrict__ tag_len, const long long *__restrict__ order, int64_t n,
                                                         int64_t byte_begin, unsigned long long *__restrict__ keys)
{
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        const int64_t u = order ? order[i] : i;
        uint64_t key = 0;
        if (u >= 0 && u < n) {
            const int64_t off = tag_off[u];
            const int32_t len = tag_len[u];
            if (tag_ok(off, len, n_bytes)) {
                const uint8_t *b = text + off + PREFIX;
                const int64_t left = len - PREFIX - byte_begin;          // bytes of the body from byte_begin on
#pragma unroll
                for (int j = 0; j < 8; ++j) key = (key << 8) | (j < left ? b[byte_begin + j] : 0u);
            }
        }
        keys[i] = key;
    }
}

// tag(a) against tag(b) as the rule orders them: -1 a first, +1 b first, 0 equal
__device__ __forceinline__ int compare_tags(const uint8_t *__restrict__ text, int64_t n_bytes, int64_t off_a, int32_t len_a, int64_t off_b,
                                            int32_t len_b)
{
    const bool ta = tag_ok(off_a, len_a, n_bytes), tb = tag_ok(off_b, len_b, n_bytes);
    if (!ta || !tb) return ta ? -1 : tb ? 1 : 0;             // untagged behind tagged, untagged equal to untagged
    const uint8_t *a = text + off_a + PREFIX, *b = text + off_b + PREFIX;
    const int la = len_a - PREFIX, lb = len_b - PREFIX, m = la < lb ? la : lb;
    int j = 0;
    for (; j + 8 <= m; j += 8) {
        uint64_t x, y;
        __builtin_memcpy(&x, a + j, 8);                      // (no alignment is promised)
        __builtin_memcpy(&y, b + j, 8);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
    }
    for (; j < m; ++j)
        if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
    return la < lb ? -1 : la > lb ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void tag_compare_kernel(const uint8_t *__restrict__ text, int64_t n_bytes, const long long *__restrict__ tag_off,
                                                            const int32_t *__restrict__ tag_len, const long long *__restrict__ order, int64_t n,
                                                            int8_t *__restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
        int r = 0;
        if (i > 0) {
            const int64_t ua = order ? order[i - 1] : i - 1, ub = order ? order[i] : i;
            const bool ia = ua >= 0 && ua < n, ib = ub >= 0 && ub < n;       // (an order that is none: such a unit counts as untagged)
            r = compare_tags(text, n_bytes, ia ? tag_off[ua] : -1, ia ? tag_len[ua] : 0, ib ? tag_off[ub] : -1, ib ? tag_len[ub] : 0);
        }
        out[i] = (int8_t)r;
    }
}

// what the three entries refuse alike: PG_OK, or PG_EINVAL with the text for pg_last_error
int check_text(const char *who, const uint8_t *text, int64_t n_bytes, int64_t n, const char *n_name)
{
    if (!text) return pg_fail(PG_EINVAL, "%s: text is null", who);
    if (n_bytes < 0) return pg_fail(PG_EINVAL, "%s: n_bytes is negative (%lld)", who, (long long)n_bytes);
    if (n < 0) return pg_fail(PG_EINVAL, "%s: %s is negative (%lld)", who, n_name, (long long)n);
    if (n > MAX_UNITS) return pg_fail(PG_EINVAL, "%s: %s %lld beyond 2^40", who, n_name, (long long)n);
    if ((uintptr_t)text & 15) return pg_fail(PG_EINVAL, "%s: text is not 16-byte aligned", who);
    return PG_OK;
}

}  // namespace

extern "C" int pg_fastq_barcode_tags(const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_units, int lines_per_unit,
                                     int64_t *tag_off, int32_t *tag_len, uint64_t *status, void *stream)
{
    const char *who = "pg_fastq_barcode_tags";
    if (!line_start) return pg_fail(PG_EINVAL, "%s: line_start is null", who);
    if (!tag_off) return pg_fail(PG_EINVAL, "%s: tag_off is null", who);
    if (!tag_len) return pg_fail(PG_EINVAL, "%s: tag_len is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    if (lines_per_unit != 4 && lines_per_unit != 8) return pg_fail(PG_EINVAL, "%s: lines_per_unit %d is neither 4 nor 8", who, lines_per_unit);
    const int rc = check_text(who, text, n_bytes, n_units, "n_units");
    if (rc) return rc;
    if (n_units == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(status + 1, 0xff, sizeof(uint64_t), s) != hipSuccess)
        return pg_fail(PG_EHIP, "%s: cannot clear the status", who);
    hipLaunchKernelGGL(barcode_tags_kernel, dim3(grid_for(n_units, WAVES)), dim3(BLOCK), 0, s, text, n_bytes, (const long long *)line_start, n_units,
                       lines_per_unit, (long long *)tag_off, tag_len, (unsigned long long *)status);
    return check_launch(who);
}

extern "C" int pg_fastq_tag_keys(const uint8_t *text, int64_t n_bytes, const int64_t *tag_off, const int32_t *tag_len, const int64_t *order,
                                 int64_t n, int64_t byte_begin, uint64_t *keys, void *stream)
{
    const char *who = "pg_fastq_tag_keys";
    if (!tag_off) return pg_fail(PG_EINVAL, "%s: tag_off is null", who);
    if (!tag_len) return pg_fail(PG_EINVAL, "%s: tag_len is null", who);
    if (!keys) return pg_fail(PG_EINVAL, "%s: keys is null", who);
    if (byte_begin < 0 || (byte_begin & 7) || byte_begin > MAX_BODY)
        return pg_fail(PG_EINVAL, "%s: byte_begin %lld is no multiple of 8 in [0, %d]", who, (long long)byte_begin, MAX_BODY);
    const int rc = check_text(who, text, n_bytes, n, "n");
    if (rc) return rc;
    if (n == 0) return PG_OK;
    hipLaunchKernelGGL(tag_keys_kernel, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, text, n_bytes, (const long long *)tag_off, tag_len,
                       (const long long *)order, n, byte_begin, (unsigned long long *)keys);
    return check_launch(who);
}

extern "C" int pg_fastq_tag_compare(const uint8_t *text, int64_t n_bytes, const int64_t *tag_off, const int32_t *tag_len, const int64_t *order,
                                    int64_t n, int8_t *out, void *stream)
{
    const char *who = "pg_fastq_tag_compare";
    if (!tag_off) return pg_fail(PG_EINVAL, "%s: tag_off is null", who);
    if (!tag_len) return pg_fail(PG_EINVAL, "%s: tag_len is null", who);
    if (!out) return pg_fail(PG_EINVAL, "%s: out is null", who);
    const int rc = check_text(who, text, n_bytes, n, "n");
    if (rc) return rc;
    if (n == 0) return PG_OK;
    hipLaunchKernelGGL(tag_compare_kernel, dim3(grid_for(n, BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, text, n_bytes, (const long long *)tag_off,
                       tag_len, (const long long *)order, n, out);
    return check_launch(who);
}
