// fastq_prep.hip -- raw stLFR and TELL-seq read pairs made into the form every entry point of this library takes, on the FASTQ
// TEXT in device memory: the barcode brought into a BX:Z: tag on both mates' headers (pangaea_amd/prepreads.py: preprocess_reads;
// sortreads.py: sort_fastq / check_fastq with short_type).  Stands beside the first half of step 0 of the reference's driver,
// src/run_pangaea:138-149 -> preprocess_stlfr.cpp:68-113 as called with -n -l, and src/run_pangaea:151-162 ->
// preprocess_tellseq.cpp:52-84; semantics: the header's section "Raw stLFR and TELL-seq read pairs brought to the BX:Z: form".
// A translation unit of its own, so that work on it cannot touch the timed kernels' code objects.  The line indices are
// pg_fastq_index's; the lengths of the new records are the caller's element-wise arithmetic on them and on the plan arrays.
//
// A known oddity that is kept: the reference tests the FIRST field of a stLFR barcode twice and never the third
// (preprocess_stlfr.cpp:89), so 5_6_0 is tagged and 5_0_7, 0_6_7 and 0_0_0 are not.
//
// Shapes, and why:
//   plan    one wavefront per unit, R1's header 64 bytes per turn, one byte per lane, every decision a ballot (a 64-bit mask in
//           scalar registers, scalar branches), as barcode_tags_kernel of fastq_sort.hip.  stLFR asks four dependent "first set
//           bit at or behind x" questions -- the leftmost '#', the leftmost '/' behind it, the first two '_' between them --
//           that may lie in different turns: what is found is kept in scalar registers (p, u1, u2, q; -1: not yet), and each
//           turn masks its ballots from the last find on (`& ~((2 << b) - 1)`, empty at b = 63) before it takes ctz.  Whether
//           f1 or f2 is the one byte '0' needs the byte BEHIND '#' and behind the first '_': the ballot of c == '0' answers in
//           the same turn, or in the next one when the find was the turn's last byte (a pending flag) -- no further load.
//           TELL-seq asks one question of the header (the first space) and none of the index read's bytes: its barcode is
//           the sequence line of I1's record, whose offset and length stand in I1's line index.  Per unit TWO dependent round
//           trips: the 5 line starts of each file, one per lane (lanes 0-4 R1, 8-12 R2, 16-20 I1); then, together, the
//           header's first turn and the '@' / '+' bytes of all two or three records.  Longer headers: one trip per turn.
//   write   one wavefront per kept unit, both mates one after the other (one wavefront per unit AND mate was measured and is
//           slower, 1.52 against 1.22 ms for 1 M stLFR pairs: the per-unit loads and checks are then made twice and the copies
//           are too short to gain from more wavefronts).  A new record is at most five pieces -- the kept head (from R1's text for
//           BOTH mates), "\tBX:Z:" + B + "-1" byte-wise (at most 8 + PG_FASTQ_MAX_TAG - 2 bytes), '\n', and the rest of the
//           mate's own record: ONE copy of lines 1 .. 3 for stLFR and for a TELL-seq record whose third line is "+\n" already
//           (every record a sequencer writes), else line 1, "+\n", line 3 --, copied as
//           fastq_gather_kernel copies (16-byte stores on the destination's alignment, unaligned loads).
//           TELL-seq's white list (B + '\n' per kept unit, 19 bytes at 19 i) is written by the same wavefront when asked for.
//           All per-unit values are loaded before the first copy; with kept == NULL (every unit, stLFR) that is two dependent
//           trips, else three.
// Plain loads and stores throughout; the status words are updated as pg_table_read_hits updates them (atomicOr / atomicMin,
// on a malformed record only).  Whatever the device arrays hold, no byte outside [0, n_bytes) of a text is read and none
// outside [0, out_bytes) of an output written.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pangaea_feat.h"
#include "pg_internal.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_B = PG_FASTQ_MAX_TAG - 2;                  // bytes of a barcode: "-1" behind it still fits the sort's limit
constexpr int TELLSEQ_B = 18;                                // preprocess_tellseq.cpp:72
constexpr int64_t MAX_UNITS = 1LL << 40;
constexpr uint64_t PREFIX_BYTES = 0x3A5A3A584209ull;         // "\tBX:Z:", the first byte lowest

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

// a 64-bit value of lane k, the same in every lane, in scalar registers
__device__ __forceinline__ int64_t from_lane(int64_t v, int k)
{
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, k), hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), k);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// the bits of m behind bit b (b = 63: none)
__device__ __forceinline__ uint64_t behind(uint64_t m, int b) { return m & ~((2ull << b) - 1); }

struct Texts {
    const uint8_t *text[3];                                  // R1, R2, I1 (TELL-seq only)
    int64_t n_bytes[3];
    const long long *line_start[3];
};

__device__ __forceinline__ void report(unsigned long long *status, int file, int64_t record, uint32_t reason)
{
    atomicMin(&status[2 * file + 1], ((unsigned long long)record << 8) | reason);
    atomicOr(&status[2 * file], (unsigned long long)PG_STATUS_FASTQ_FORMAT);
}

__global__ __launch_bounds__(BLOCK) void prep_plan_kernel(Texts t, int mode, int64_t n_units, int64_t first_unit, long long *__restrict__ head_len,
                                                          long long *__restrict__ bc_off, int32_t *__restrict__ bc_len,
                                                          uint8_t *__restrict__ tagged, unsigned long long *status)
{
    const int lane = threadIdx.x & 63;
    // (the wavefront's number in a form the compiler knows to be the same in every lane: what follows from it stays scalar)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    const int n_files = mode == PG_PREP_TELLSEQ ? 3 : 2;
    const int file = lane >> 3, line = lane & 7;             // lane 8 f + k: line k of this unit's record in file f
    const bool holds = file < n_files && line <= 4;
    // (selects, not an index that differs between lanes into the argument block)
    const long long *const my_index = file == 1 ? t.line_start[1] : file == 2 ? t.line_start[2] : t.line_start[0];
    const uint8_t *const my_text = file == 1 ? t.text[1] : file == 2 ? t.text[2] : t.text[0];
    const int64_t my_bytes = file == 1 ? t.n_bytes[1] : file == 2 ? t.n_bytes[2] : t.n_bytes[0];
    const uint8_t *const text1 = t.text[0];
    for (int64_t u = (int64_t)blockIdx.x * WAVES + wave; u < n_units; u += n_waves) {
        const int64_t mine = holds ? my_index[4 * u + line] : 0;
        const int64_t next = __shfl_down(mine, 1);
        // line k of a record begins in front of line k + 1 (its last line may be empty: the text's end), inside [0, n_bytes]
        const bool in_order = line == 3 ? mine <= next : mine < next;
        const uint64_t off_index = __ballot(holds && ((line < 4 && !in_order) || (line == 0 && mine < 0) || (line == 4 && mine > my_bytes)));
        bool bad = false;
        int64_t head = 0, b_off = -1, b_len = 0;
        bool tag = false;
        if (off_index) {                                     // (no index of these texts: nothing of a text is read)
            for (int f = 0; f < n_files; ++f)
                if (lane == 0 && ((off_index >> (8 * f)) & 0xff)) report(status, f, first_unit + u, PG_FASTQ_BAD_INDEX);
            bad = true;
        } else {
            const int64_t a = from_lane(mine, 0), e = from_lane(mine, 1) - 1;        // R1's header without its '\n': 0 <= a <= e < n_bytes
            const bool marks = holds && (line == 0 || line == 2);                    // (every line 0 and 2 begins below its text's end)
            const uint32_t marker = marks ? my_text[mine] : 0;
            uint32_t c = a + lane < e ? text1[a + lane] : 0;                         // (behind the content: NUL, which is none of the bytes asked for)
            const uint64_t off_marker = __ballot(marks && marker != (line ? '+' : '@'));
            if (off_marker) {
                for (int f = 0; f < n_files; ++f) {
                    const uint32_t m = (uint32_t)(off_marker >> (8 * f)) & 0xff;     // bit 0: no '@', bit 2: no '+'
                    if (lane == 0 && m) report(status, f, first_unit + u, (m & 1) ? PG_FASTQ_NO_AT : PG_FASTQ_NO_PLUS);
                }
                bad = true;
            } else if (mode == PG_PREP_TELLSEQ) {
                int64_t s = e;                               // the first space, or the end
                for (int64_t p0 = a;;) {
                    const uint64_t sp = __ballot(c == ' ');
                    if (sp) { s = p0 + __builtin_ctzll(sp); break; }
                    p0 += 64;
                    if (p0 >= e) break;
                    c = p0 + lane < e ? text1[p0 + lane] : 0;
                }
                head = s - a;
                b_off = from_lane(mine, 17);                 // the sequence line of I1's record, without its '\n'
                const int64_t len = from_lane(mine, 18) - 1 - b_off;
                b_len = len > INT32_MAX ? INT32_MAX : len;
                tag = len == TELLSEQ_B;
            } else {
                int64_t p = -1, u1 = -1, u2 = -1, q = -1;    // '#', the first two '_' behind it, the first '/' behind it
                uint32_t z1 = 0, z2 = 0;                     // the byte behind '#' / behind the first '_' is '0'
                bool pend1 = false, pend2 = false;           // ... and that byte is the next turn's first
                for (int64_t p0 = a; p0 < e;) {
                    uint64_t ms = __ballot(c == '/'), mu = __ballot(c == '_');
                    const uint64_t m0 = __ballot(c == '0');
                    if (pend1) { z1 = (uint32_t)(m0 & 1); pend1 = false; }
                    if (pend2) { z2 = (uint32_t)(m0 & 1); pend2 = false; }
                    bool look = true;
                    if (p < 0) {
                        const uint64_t mh = __ballot(c == '#');
                        if (mh) {
                            const int b = __builtin_ctzll(mh);
                            p = p0 + b;
                            ms = behind(ms, b);
                            mu = behind(mu, b);
                            if (b < 63) z1 = (uint32_t)(m0 >> (b + 1)) & 1; else pend1 = true;
                        } else look = false;
                    }
                    if (look) {
                        if (ms) {                            // the barcode ends here: only what stands in front of it counts
                            const int b = __builtin_ctzll(ms);
                            q = p0 + b;
                            mu &= (1ull << b) - 1;
                        }
                        if (u1 < 0 && mu) {
                            const int b = __builtin_ctzll(mu);
                            u1 = p0 + b;
                            mu = behind(mu, b);
                            if (b < 63) z2 = (uint32_t)(m0 >> (b + 1)) & 1; else pend2 = true;
                        }
                        if (u1 >= 0 && u2 < 0 && mu) u2 = p0 + __builtin_ctzll(mu);
                        if (q >= 0) break;
                    }
                    p0 += 64;
                    if (p0 >= e) break;
                    c = p0 + lane < e ? text1[p0 + lane] : 0;
                }
                if (q < 0) q = e;                            // no '/': the barcode goes to the header's end
                const uint32_t why = p < 0 ? PG_FASTQ_NO_HASH : u2 < 0 ? PG_FASTQ_FEW_FIELDS : q - p - 1 > MAX_B ? PG_FASTQ_LONG_TAG : 0;
                if (why) {
                    if (lane == 0) report(status, 0, first_unit + u, why);
                    bad = true;
                } else {
                    head = p - a;
                    b_off = p + 1;
                    b_len = q - p - 1;
                    // tagged iff neither f1 nor f2 is the string "0"; f3 is never asked (preprocess_stlfr.cpp:89)
                    tag = !(u1 - p - 1 == 1 && z1) && !(u2 - u1 - 1 == 1 && z2);
                }
            }
        }
        if (lane == 0) {
            head_len[u] = bad ? 0 : head;
            bc_off[u] = bad ? -1 : b_off;
            bc_len[u] = bad ? 0 : (int32_t)b_len;
            tagged[u] = !bad && tag;
        }
    }
}

// len bytes from src to dst by one wavefront (the caller has checked both ranges): the destination side in whole 16-byte
// pieces, each read from wherever it lies in the source, the fewer than 16 bytes in front and behind byte-wise
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, int64_t len, int lane)
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

// the four line starts and the end of record u: inside the text and in order (the last line may be empty: the text's end)
__device__ __forceinline__ bool record_of(const long long *__restrict__ ls, int64_t u, int64_t n_bytes, int64_t *s)
{
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = ls[4 * u + k];
    return s[0] >= 0 && s[0] < s[1] && s[1] < s[2] && s[2] < s[3] && s[3] <= s[4] && s[4] <= n_bytes;
}

__global__ __launch_bounds__(BLOCK) void prep_write_kernel(Texts t, int mode, int64_t n_units, const long long *__restrict__ head_len,
                                                           const long long *__restrict__ bc_off, const int32_t *__restrict__ bc_len,
                                                           const uint8_t *__restrict__ tagged, const long long *__restrict__ kept,
                                                           const long long *__restrict__ dst1, const long long *__restrict__ dst2, int64_t n_kept,
                                                           uint8_t *out1, int64_t out1_bytes, uint8_t *out2, int64_t out2_bytes,
                                                           uint8_t *__restrict__ white_list, int64_t white_list_bytes)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));    // (scalar loads of what is per unit)
    const int64_t n_waves = (int64_t)gridDim.x * WAVES;
    const bool tell = mode == PG_PREP_TELLSEQ;
    const uint8_t *const bc_text = t.text[tell ? 2 : 0];
    const int64_t bc_bytes = t.n_bytes[tell ? 2 : 0];
    for (int64_t i = (int64_t)blockIdx.x * WAVES + wave; i < n_kept; i += n_waves) {
        const int64_t u = kept ? kept[i] : i;
        const int64_t d[2] = {dst1[i], dst2[i]};
        if (u < 0 || u >= n_units) continue;
        int64_t s[2][5];
        const bool ok1 = record_of(t.line_start[0], u, t.n_bytes[0], s[0]), ok2 = record_of(t.line_start[1], u, t.n_bytes[1], s[1]);
        const int64_t head = head_len[u], b_off = bc_off[u];
        const int b_len = bc_len[u];
        const bool tag = tagged[u] != 0;
        if (!ok1 || !ok2 || head < 0 || head > s[0][1] - 1 - s[0][0]) continue;
        if (tag && (b_off < 0 || b_len < 0 || b_len > MAX_B || b_off > bc_bytes - b_len)) continue;
        if (tell && !tag) continue;                          // (a dropped unit is not the caller's to keep)
        // (the last byte of each mate's record and the first of its third line lie inside its text, s0 < s2 < s4: loaded
        // together, no load waits behind a branch on another)
        const uint32_t last[2] = {t.text[0][s[0][4] - 1], t.text[1][s[1][4] - 1]};
        const uint32_t third[2] = {t.text[0][s[0][2]], t.text[1][s[1][2]]};
        const int64_t mid = tag ? 8 + b_len : 0;             // "\tBX:Z:" + B + "-1"
        int64_t size[2];
        bool fits = true;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int nl = (s[m][4] == s[m][3]) | (last[m] != '\n');         // a last line without its '\n' gets one
            size[m] = head + mid + 1 + (tell ? (s[m][2] - s[m][1]) + 2 + (s[m][4] - s[m][3]) : s[m][4] - s[m][1]) + nl;
            const int64_t room = m ? out2_bytes : out1_bytes;
            fits = fits && d[m] >= 0 && d[m] <= room - size[m];
        }
        if (!fits) continue;
        if (white_list && b_len == TELLSEQ_B && i <= white_list_bytes / (TELLSEQ_B + 1) - 1) {     // (TELL-seq only: the entry refuses it otherwise)
            uint8_t *const w = white_list + i * (TELLSEQ_B + 1);
            if (lane <= TELLSEQ_B) w[lane] = lane < TELLSEQ_B ? bc_text[b_off + lane] : '\n';
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            uint8_t *const o = (m ? out2 : out1) + d[m];
            const uint8_t *const text = t.text[m];
            wave_copy(o, t.text[0] + s[0][0], head, lane);
            for (int64_t j = lane; j < mid; j += 64)         // (mid is 0 for an untagged unit)
                o[head + j] = j < 6 ? (uint8_t)(PREFIX_BYTES >> (8 * j)) : j < 6 + b_len ? bc_text[b_off + j - 6] : j == 6 + b_len ? '-' : '1';
            uint8_t *const rest = o + head + mid + 1;
            if (tell && !(s[m][3] - s[m][2] == 2 && third[m] == '+')) {      // a third line that is not "+\n" already: "+\n" between lines 1 and 3
                const int64_t l1 = s[m][2] - s[m][1], l3 = s[m][4] - s[m][3];
                wave_copy(rest, text + s[m][1], l1, lane);
                wave_copy(rest + l1 + 2, text + s[m][3], l3, lane);
                if (lane < 2) rest[l1 + lane] = lane ? '\n' : '+';
            } else {
                wave_copy(rest, text + s[m][1], s[m][4] - s[m][1], lane);
            }
            if (lane == 0) {
                o[head + mid] = '\n';
                o[size[m] - 1] = '\n';                       // (the record's own last byte, or the one it lacked)
            }
        }
    }
}

// what both entries refuse alike: PG_OK, or PG_EINVAL with the text for pg_last_error
int check_texts(const char *who, int mode, const uint8_t *const *text, const int64_t *n_bytes, const int64_t *const *line_start, bool need_index_i,
                int64_t n_units)
{
    static const char *const names[3] = {"1", "2", "_i"};
    if (mode != PG_PREP_STLFR && mode != PG_PREP_TELLSEQ) return pg_fail(PG_EINVAL, "%s: mode %d is neither PG_PREP_STLFR nor PG_PREP_TELLSEQ", who, mode);
    for (int f = 0; f < 3; ++f) {
        if (f == 2 && mode != PG_PREP_TELLSEQ) {
            if (text[f] || line_start[f]) return pg_fail(PG_EINVAL, "%s: text_i and line_start_i go with PG_PREP_TELLSEQ only", who);
            continue;
        }
        if (!text[f]) return pg_fail(PG_EINVAL, "%s: text%s is null", who, names[f]);
        if ((f < 2 || need_index_i) && !line_start[f]) return pg_fail(PG_EINVAL, "%s: line_start%s is null", who, names[f]);
        if (n_bytes[f] < 0) return pg_fail(PG_EINVAL, "%s: n%s_bytes is negative (%lld)", who, names[f], (long long)n_bytes[f]);
        if ((uintptr_t)text[f] & 15) return pg_fail(PG_EINVAL, "%s: text%s is not 16-byte aligned", who, names[f]);
    }
    if (n_units < 0) return pg_fail(PG_EINVAL, "%s: n_units is negative (%lld)", who, (long long)n_units);
    if (n_units > MAX_UNITS) return pg_fail(PG_EINVAL, "%s: n_units %lld beyond 2^40", who, (long long)n_units);
    return PG_OK;
}

Texts texts_of(int mode, const uint8_t *const *text, const int64_t *n_bytes, const int64_t *const *line_start)
{
    Texts t;
    for (int f = 0; f < 3; ++f) {
        const bool on = f < 2 || mode == PG_PREP_TELLSEQ;
        t.text[f] = on ? text[f] : nullptr;
        t.n_bytes[f] = on ? n_bytes[f] : 0;
        t.line_start[f] = on ? (const long long *)line_start[f] : nullptr;
    }
    return t;
}

}  // namespace

extern "C" int pg_fastq_prep_plan(int mode, const uint8_t *text1, int64_t n1_bytes, const int64_t *line_start1, const uint8_t *text2, int64_t n2_bytes,
                                  const int64_t *line_start2, const uint8_t *text_i, int64_t n_i_bytes, const int64_t *line_start_i, int64_t n_units,
                                  int64_t first_unit, int64_t *head_len, int64_t *bc_off, int32_t *bc_len, uint8_t *tagged, uint64_t *status,
                                  void *stream)
{
    const char *who = "pg_fastq_prep_plan";
    const uint8_t *const text[3] = {text1, text2, text_i};
    const int64_t n_bytes[3] = {n1_bytes, n2_bytes, n_i_bytes};
    const int64_t *const line_start[3] = {line_start1, line_start2, line_start_i};
    const int rc = check_texts(who, mode, text, n_bytes, line_start, true, n_units);
    if (rc) return rc;
    if (first_unit < 0 || first_unit > MAX_UNITS) return pg_fail(PG_EINVAL, "%s: first_unit %lld outside [0, 2^40]", who, (long long)first_unit);
    if (!head_len) return pg_fail(PG_EINVAL, "%s: head_len is null", who);
    if (!bc_off) return pg_fail(PG_EINVAL, "%s: bc_off is null", who);
    if (!bc_len) return pg_fail(PG_EINVAL, "%s: bc_len is null", who);
    if (!tagged) return pg_fail(PG_EINVAL, "%s: tagged is null", who);
    if (!status) return pg_fail(PG_EINVAL, "%s: status is null", who);
    if (n_units == 0) return PG_OK;
    hipStream_t s = (hipStream_t)stream;
    for (int f = 0; f < 3; ++f)
        if (hipMemsetAsync(status + 2 * f, 0, sizeof(uint64_t), s) != hipSuccess || hipMemsetAsync(status + 2 * f + 1, 0xff, sizeof(uint64_t), s) != hipSuccess)
            return pg_fail(PG_EHIP, "%s: cannot clear the status", who);
    hipLaunchKernelGGL(prep_plan_kernel, dim3(grid_for(n_units, WAVES)), dim3(BLOCK), 0, s, texts_of(mode, text, n_bytes, line_start), mode, n_units,
                       first_unit, (long long *)head_len, (long long *)bc_off, bc_len, tagged, (unsigned long long *)status);
    return check_launch(who);
}

extern "C" int pg_fastq_prep_write(int mode, const uint8_t *text1, int64_t n1_bytes, const int64_t *line_start1, const uint8_t *text2, int64_t n2_bytes,
                                   const int64_t *line_start2, const uint8_t *text_i, int64_t n_i_bytes, int64_t n_units, const int64_t *head_len,
                                   const int64_t *bc_off, const int32_t *bc_len, const uint8_t *tagged, const int64_t *kept, const int64_t *dst1,
                                   const int64_t *dst2, int64_t n_kept, uint8_t *out1, int64_t out1_bytes, uint8_t *out2, int64_t out2_bytes,
                                   uint8_t *white_list, int64_t white_list_bytes, void *stream)
{
    const char *who = "pg_fastq_prep_write";
    const uint8_t *const text[3] = {text1, text2, text_i};
    const int64_t n_bytes[3] = {n1_bytes, n2_bytes, n_i_bytes};
    const int64_t *const line_start[3] = {line_start1, line_start2, nullptr};
    const int rc = check_texts(who, mode, text, n_bytes, line_start, false, n_units);
    if (rc) return rc;
    if (!head_len) return pg_fail(PG_EINVAL, "%s: head_len is null", who);
    if (!bc_off) return pg_fail(PG_EINVAL, "%s: bc_off is null", who);
    if (!bc_len) return pg_fail(PG_EINVAL, "%s: bc_len is null", who);
    if (!tagged) return pg_fail(PG_EINVAL, "%s: tagged is null", who);
    if (!dst1) return pg_fail(PG_EINVAL, "%s: dst1 is null", who);
    if (!dst2) return pg_fail(PG_EINVAL, "%s: dst2 is null", who);
    if (!out1) return pg_fail(PG_EINVAL, "%s: out1 is null", who);
    if (!out2) return pg_fail(PG_EINVAL, "%s: out2 is null", who);
    if (out1_bytes < 0) return pg_fail(PG_EINVAL, "%s: out1_bytes is negative (%lld)", who, (long long)out1_bytes);
    if (out2_bytes < 0) return pg_fail(PG_EINVAL, "%s: out2_bytes is negative (%lld)", who, (long long)out2_bytes);
    if (white_list && mode != PG_PREP_TELLSEQ) return pg_fail(PG_EINVAL, "%s: white_list goes with PG_PREP_TELLSEQ only", who);
    if (white_list && white_list_bytes < 0) return pg_fail(PG_EINVAL, "%s: white_list_bytes is negative (%lld)", who, (long long)white_list_bytes);
    if (n_kept < 0 || n_kept > n_units) return pg_fail(PG_EINVAL, "%s: n_kept %lld outside [0, n_units = %lld]", who, (long long)n_kept, (long long)n_units);
    if (n_kept == 0) return PG_OK;
    hipLaunchKernelGGL(prep_write_kernel, dim3(grid_for(n_kept, WAVES)), dim3(BLOCK), 0, (hipStream_t)stream, texts_of(mode, text, n_bytes, line_start), mode,
                       n_units, (const long long *)head_len, (const long long *)bc_off, bc_len, tagged, (const long long *)kept, (const long long *)dst1,
                       (const long long *)dst2, n_kept, out1, out1_bytes, out2, out2_bytes, white_list, white_list ? white_list_bytes : 0);
    return check_launch(who);
}
