/*
 * pangaea_feat.h -- C ABI of libpangaea_feat.so, the MI355X (gfx950) implementation of Pangaea's
 * barcode-aware k-mer feature path.
 *
 * The reference has no in-process FFI on this path: src/feature.py shells out to two binaries
 * (count_tnf, count_kmer) and to jellyfish, and reads their CSV files back.  This header is the
 * boundary a maintainer binds instead (ctypes stub in INTEGRATION.md).  Every entry point names the
 * reference interface it replaces.  Conventions:
 *   - plain pointers and sizes only; no C++ or torch types;
 *   - every function returns PG_OK (0) or a negative pg_status; pg_last_error() gives the message of the
 *     last failure on the calling thread; nothing here calls exit();
 *   - "device" pointers are HIP device pointers owned by the caller (e.g. torch tensors' data_ptr());
 *     `stream` is a hipStream_t passed as void* (NULL = the null stream).  Device functions only enqueue
 *     work on `stream`; they never allocate, free or synchronise;
 *   - host handles (pg_reads) are owned by the library until the matching free.
 *
 * Read-stream layout (host and device): the text the reference accumulates per barcode run --
 * read1 + 'N' + read2 + 'N' per pair (count_tnf.cpp:248,251) -- is kept for the WHOLE file as one
 * character stream in file order.  Character j lives in
 *     codes[j / 32] bits [2*(j%32), 2*(j%32)+2)   A=0 C=1 T=2 G=3   (count_tnf.cpp:99: (c>>1)&3)
 *     valid[j / 32] bit  (j % 32)                  1 iff the character is one of 'A','C','G','T'
 * Separators, N, lower-case and IUPAC characters have valid=0 (and code 0).  Arrays are padded with
 * invalid characters to a whole number of PG_WORD_ALIGN words.  A barcode run is a contiguous
 * character range of the stream, so rows never need per-read offsets.
 */
#ifndef PANGAEA_FEAT_H
#define PANGAEA_FEAT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 9   /* 9: pg_ingest_fastq_pair_device / pg_ingest_place_pair (-1 / -2 input with the device copy inside);
                              8: pg_inflate_to_memfd (gzip input for the ingest with the device copy inside);
                              7: pg_build_flags (what kind of build a loaded library is), pg_mini_gather_entries names its buffer's size,
                                 pg_mini_shuffle_bytes_merged, a stream counted in pieces (pg_mini_count_piece / pg_mini_lookup_*);
                              6: pg_ingest_fastq_device / pg_ingest_place (ingest with the device copy inside);
                              5: pg_mini_count takes the merged lookups' word buffer (pg_mini_merge_words), the multi-rank half entries;
                              4: pg_mini_records_bytes takes the table, status bits;
                              3: PG_TABLE_MINI and the super-k-mer entry points; 2: packed hash slots keyed by pg_key42(code) */
#define PG_CHARS_PER_WORD 32
#define PG_WORD_ALIGN 256 /* stream arrays are padded to a multiple of this many words */

typedef enum {
    PG_OK = 0,
    PG_EINVAL = -1,      /* bad argument (unsupported k, null pointer, ...) */
    PG_EIO = -2,         /* cannot open / read / write a file */
    PG_EFORMAT = -3,     /* input the reference itself would abort on (header ending in a bare "BX:Z") */
    PG_ENOMEM = -4,
    PG_EHIP = -5,        /* a HIP runtime call or kernel launch failed */
    PG_ETABLEFULL = -6,  /* hash table too small: enlarge log2_slots and count again */
    PG_ENODEVICE = -7    /* no gfx950 device / code object not loadable */
} pg_status;

int pg_abi_version(void);
/* What kind of build this library is -- 0 for the product (libpangaea_feat.so as `make` builds it).  A loader refuses anything
 * else unless it asked for it: a checked library is slower, a variant may compute WRONG results (timing experiments).
 *   PG_BUILD_CHECKED  the super-k-mer kernels check every global store against its buffer's capacity (PG_STATUS_BOUNDS)
 *   PG_BUILD_STAMPS   phase timers inside the bucket kernels (-DPG_MINI_STAMPS)
 *   PG_BUILD_VARIANT  built with extra compiler flags (`make variant NAME=... KFLAGS=...`): not the product, whatever it does */
#define PG_BUILD_CHECKED 1u
#define PG_BUILD_STAMPS 2u
#define PG_BUILD_VARIANT 4u
uint32_t pg_build_flags(void);
const char *pg_last_error(void);
/* number of visible HIP devices, or a negative pg_status */
int pg_device_count(void);

/* ----------------------------------------------------------------------------------------------
 * Host ingest: FASTQ -> read stream + barcode runs.
 * Replaces the single-threaded producer loops of count_tnf.cpp:174-289 and count_kmer.cpp:186-281
 * together with getBarcode (count_tnf.cpp:23-52).  r2 == NULL selects the interleaved form (-i),
 * otherwise r1/r2 are the -1/-2 files.  gzip or plain, as gzstream's gzopen.
 * Runs are assembled exactly as the reference does (the pair is appended before the barcode
 * comparison), so run i = [run_off[i], run_off[i+1]) in characters.  Reads that jellyfish counts but
 * that belong to no run (paired mode, name/barcode mismatch, count_tnf.cpp:183) are placed after the
 * last run, in [run_off[n_runs], n_chars).
 * ---------------------------------------------------------------------------------------------- */
typedef struct pg_reads pg_reads;

int pg_ingest_fastq(const char *r1_or_interleaved, const char *r2_or_null, pg_reads **out);
/* Threads the interleaved parser may use (0 = all hardware threads, at most 32; PG_INGEST_THREADS overrides the
 * default).  The result does not depend on it. */
void pg_set_ingest_threads(int n);
/* Sharded ingest, one shard per rank/GPU (contiguous ranges of barcode runs): shard `part` of `n_parts`
 * parses only its byte range [size*part/n_parts, size*(part+1)/n_parts) of an UNCOMPRESSED interleaved file, moved
 * forward at both ends to the end of the barcode run in progress there, so that the shards' runs concatenated in
 * rank order are exactly the runs pg_ingest_fastq gives for the whole file (the producer loop of
 * count_tnf.cpp:238-289 is inherently serial; this is its data-parallel form).  Record alignment comes from line
 * numbers, not from guessing at '@': first every rank calls pg_fastq_count_newlines for its own range, the counts
 * are exchanged, and newlines_before[i] (i = 0..n_parts) = number of '\n' in bytes [0, size*i/n_parts).  gzip input
 * fails with PG_EFORMAT (callers fall back to pg_ingest_fastq on every rank). */
int pg_fastq_count_newlines(const char *path, int part, int n_parts, int64_t *n_newlines);
int pg_ingest_fastq_shard(const char *path, int part, int n_parts, const int64_t *newlines_before, pg_reads **out);
/* The same two ingests with the copy to the GPU inside (ingest_dev.hip; replaces count_tnf.cpp:234-283 + the device copy for
 * uncompressed interleaved input): the byte range is cut into pieces (PG_INGEST_PIECE bytes, default 16 MiB) that the parser
 * threads take from a queue; a thread copies the packed characters of a piece it has finished into the device STAGING arrays
 * while the other threads go on parsing, so the PCIe copy hides under the parse, and the last host phase -- shifting every
 * piece to its bit offset in the stream -- becomes one kernel: pg_ingest_place writes codes[n_words] / valid[n_words]
 * (n_words = pg_reads_n_words) from the staging arrays.  No host copy of the stream exists: pg_reads_codes / pg_reads_valid
 * of such a handle are NULL; runs, names, counts and the (host, rare) lower-case plane are as for pg_ingest_fastq.
 * part / n_parts / newlines_before as for pg_ingest_fastq_shard (0 / 1 / NULL: the whole file).  staging_codes
 * (uint64) and staging_valid (uint32) are DEVICE arrays of staging_words >= pg_ingest_staging_words(file size) elements, free
 * again after pg_ingest_place.  *out stays NULL with status PG_OK when the input is not an uncompressed file: the caller then
 * uses pg_ingest_fastq and copies the arrays itself.  The stream is identical to pg_ingest_fastq's for every piece size. */
int64_t pg_ingest_staging_words(int64_t file_bytes);
/* gzip input for the device ingest (feature.py:76-91 reads *.gz through `pigz -dc`: one inflate stream): the file is inflated
 * into an anonymous in-memory file, as pg_ingest_fastq does for its threaded parse; *fd_out is then a descriptor that
 * "/proc/self/fd/<fd>" names for pg_ingest_fastq_device (*bytes_out = the size of the text, for pg_ingest_staging_words) and
 * that the caller closes.  *fd_out = -1 with status PG_OK: not a gzip file, or its text does not fit the memory this process
 * may park it in (PG_INFLATE_MAX_BYTES; half of what is available by default) -- the caller takes pg_ingest_fastq, which
 * then streams it. */
int pg_inflate_to_memfd(const char *path, int *fd_out, int64_t *bytes_out);
int pg_ingest_fastq_device(const char *path, int part, int n_parts, const int64_t *newlines_before, int64_t file_bytes,
                           uint64_t *staging_codes, uint32_t *staging_valid, int64_t staging_words, pg_reads **out);
int pg_ingest_place(const pg_reads *r, uint64_t *staging_codes, const uint32_t *staging_valid, int64_t staging_words,
                    uint64_t *codes, uint32_t *valid, int64_t n_words, void *stream);
/* The same for -1 / -2 input (count_tnf.cpp:174-231, the paired loop: a pair whose names or barcodes differ is skipped, its reads
 * follow the last run; feature.py:76-83: bases of a quality below '?' are not bases to jellyfish -- the low-quality plane):
 * R1 is cut into pieces of PG_INGEST_PIECE bytes, a thread that has paired and packed the records of a piece (and found the
 * same records in R2) copies its local streams -- codes, validity, low quality -- into the three device STAGING arrays while
 * the others go on, and pg_ingest_place_pair shifts the pieces into place: codes, valid and -- if pg_reads_staged_lowq --
 * lowq[n_words] (pg_reads_lowq of such a handle is NULL: the plane exists on the device only).  staging_words >=
 * pg_ingest_pair_staging_words(bytes of R1, bytes of R2).  *out stays NULL with status PG_OK when the two are not
 * uncompressed files (gzip: pg_inflate_to_memfd first): the caller then uses pg_ingest_fastq.  Same stream, runs and counters
 * as pg_ingest_fastq(r1, r2) for every piece size and thread count. */
int64_t pg_ingest_pair_staging_words(int64_t r1_bytes, int64_t r2_bytes);
int pg_ingest_fastq_pair_device(const char *r1, const char *r2, int64_t r1_bytes, int64_t r2_bytes, uint64_t *staging_codes,
                                uint32_t *staging_valid, uint32_t *staging_lowq, int64_t staging_words, pg_reads **out);
int pg_reads_staged_lowq(const pg_reads *r);
int pg_ingest_place_pair(const pg_reads *r, uint64_t *staging_codes, const uint32_t *staging_valid, const uint32_t *staging_lowq,
                         int64_t staging_words, uint64_t *codes, uint32_t *valid, uint32_t *lowq, int64_t n_words, void *stream);
void pg_reads_free(pg_reads *r);
int64_t pg_reads_n_chars(const pg_reads *r);
int64_t pg_reads_n_words(const pg_reads *r); /* padded word count of codes[] and valid[] */
int64_t pg_reads_n_pairs(const pg_reads *r);
int64_t pg_reads_n_unpaired(const pg_reads *r);
int64_t pg_reads_n_runs(const pg_reads *r);
const uint64_t *pg_reads_codes(const pg_reads *r);
const uint32_t *pg_reads_valid(const pg_reads *r);
/* NULL, or the plane of LOWER-case a c g t (same layout as valid) when the input has any: jellyfish counts them as bases
 * (feature.py:94), the reference's own counters reset on them (count_tnf.cpp:91-96) -- so `valid` excludes them, their
 * codes are in `codes` all the same, and a caller that wants jellyfish's table counts with valid | lower (and gives the
 * strict plane in pg_rows.strict_valid). */
const uint32_t *pg_reads_lower(const pg_reads *r);
/* NULL, or the plane of bases (either case) whose quality character is below '?' -- paired (-1/-2) input only: there the
 * reference runs jellyfish with --min-qual-char=? (feature.py:76-83), which counts such bases as N, while count_tnf /
 * count_kmer never read the quality lines.  The multiplicity table is therefore counted with (valid | lower) & ~lowq and
 * the rows with `valid`: a row's k-mer may be missing from the table (count_kmer.cpp:87 skips it), so these inputs take
 * the lookup form of pg_features. */
const uint32_t *pg_reads_lowq(const pg_reads *r);
const int64_t *pg_reads_run_off(const pg_reads *r); /* [n_runs + 1] */
const char *pg_reads_run_name(const pg_reads *r, int64_t i);
/* every run name followed by a NUL into out[0 .. cap); returns the bytes needed (cap = 0, out = NULL: size only) */
int64_t pg_reads_run_names(const pg_reads *r, char *out, int64_t cap);
/* "" (undecided), "10x" or "stLFR": the header mode the file latched (count_tnf.cpp:27-32) */
const char *pg_reads_mode(const pg_reads *r);
/* Surviving rows: runs with a non-empty barcode and more than min_len characters
 * (count_tnf.cpp:81 == count_kmer.cpp:62).  row_run may be NULL to obtain only the count. */
int64_t pg_reads_rows(const pg_reads *r, int min_len, int64_t *row_run);

/* ASCII run text -> stream words (the packing used by pg_ingest_fastq, exposed for callers that
 * already hold reads in memory).  codes/valid must hold pg_words_for(n) words. */
int64_t pg_words_for(int64_t n_chars);
int pg_pack_ascii(const char *text, int64_t n_chars, uint64_t *codes, uint32_t *valid);
/* the same with the lower-case plane (may be NULL); returns 1 if the text has lower-case bases, 0 if not */
int pg_pack_ascii_lower(const char *text, int64_t n_chars, uint64_t *codes, uint32_t *valid, uint32_t *lower);

/* Split rows into work segments of at most seg_chars characters (a multiple of 32).  Call with
 * seg_row == NULL to obtain the number of segments.  Host arrays. */
int64_t pg_plan_segments(const int64_t *row_start, const int64_t *row_end, int64_t n_rows, int64_t seg_chars,
                         int32_t *seg_row, int64_t *seg_start, int64_t *seg_end);

/* ----------------------------------------------------------------------------------------------
 * TNF columns.  Column c of a TNF row counts the canonical k-mer with the c-th smallest code
 * (std::map iteration order, count_tnf.cpp:108-109).  colmap[code] (4^k entries) gives the column of
 * min(code, revcomp(code)).
 * ---------------------------------------------------------------------------------------------- */
#define PG_TNF_MAX_K 6
int pg_tnf_ncols(int k);
int pg_tnf_colmap(int k, uint16_t *colmap /* [4^k] host */, uint32_t *col_code /* [ncols] host, may be NULL */);

/* ----------------------------------------------------------------------------------------------
 * Global canonical k-mer multiplicities over every read (device).
 * Replaces `jellyfish count -C -m k` + `jellyfish dump` (src/feature.py:94,103) and the dump reload
 * of count_kmer.cpp:139-170.  Two table forms:
 *   PG_TABLE_DENSE  k <= 16: uint32_t counts[4^k], indexed by the canonical code.
 *   PG_TABLE_HASH   k <= 21: uint64_t slots[2^log2_slots], open addressing, linear probing;
 *                   slot = (key << 22) | count, 0 = empty, where key = pg_key42(canonical code) is a
 *                   BIJECTION of the 42-bit codes onto themselves that mixes like a hash (below): a k-mer is
 *                   hashed once and its key then serves as bucket id (top bits), slot index (the bits
 *                   under them) and identity.  The count field stops growing at PG_HASH_COUNT_SAT (2^21),
 *                   far above any vector_size*window, so every histogram bin is exact.  A key's home slot
 *                   is its top log2_slots bits.  With log2_bucket_slots = b > 0 the table
 *                   is split into buckets of 2^b consecutive slots and probing wraps inside the
 *                   bucket (b = 0: one bucket = the whole table); pg_kmer_count_bucketed needs
 *                   b <= PG_BUCKET_MAX_LOG2_SLOTS so that one bucket fits in LDS.
 *   PG_TABLE_WIDE   k <= 31 (the reference's whole range, count_kmer.cpp:11-21): uint64_t keys[2^log2_slots]
 *                   holding code + 1 (0 = empty), immediately followed by uint32_t counts[2^log2_slots]
 *                   (12 bytes per slot); same placement and probing, unbucketed, built and read by the direct
 *                   kernels (pg_kmer_count / pg_features) only; counts are plain uint32 (no saturation).
 * Tables must be zero-filled by the caller before the first count; counting accumulates, so a stream
 * may be counted in pieces (and tables of several GPUs can be summed).
 * ---------------------------------------------------------------------------------------------- */
enum { PG_TABLE_DENSE = 1, PG_TABLE_HASH = 2, PG_TABLE_WIDE = 3, PG_TABLE_MINI = 4, PG_TABLE_MINI_WIDE = 5 };
/*   PG_TABLE_MINI   PG_MINI_MIN_K <= k <= 21: uint64_t slots[2^log2_slots], slot = (canonical code << 22) | count, in
 *                   buckets of 2^log2_bucket_slots slots (<= PG_BUCKET_MAX_LOG2_SLOTS, at most 2^16 buckets); a k-mer's
 *                   bucket is a hash of its MINIMIZER (the smallest hashed canonical 13-mer inside it; 11-mer for k < 16), its home slot
 *                   inside the bucket a hash of its code; linear probing wraps inside the bucket.  Consecutive k-mers
 *                   of a read share their minimizer, so the partition passes move super-k-mers (12 bytes for a run of
 *                   k-mers) instead of 8 bytes per occurrence: built by pg_mini_plan + pg_mini_count, read by
 *                   pg_features (lookups) and pg_kmer_merge (entries of a dump).
 *   PG_TABLE_MINI_WIDE  22 <= k <= 31, the same pipeline with the slot layout of PG_TABLE_WIDE: uint64_t keys[2^log2_slots]
 *                   (canonical code + 1, 0 = empty) followed by uint32_t counts[2^log2_slots] (plain 32-bit counts, no
 *                   saturation value); buckets of <= 2^PG_MINI_WIDE_MAX_LOG2_BUCKET_SLOTS slots (12 bytes per slot in
 *                   LDS).  The minimizer is taken over the CENTRAL 8 or 9 13-mers of the k-mer (a window that the
 *                   reverse complement maps onto itself), so the first pass keeps at most 9 values per lane for every k.
 *                   Entries of a dump are merged with pg_kmer_merge_wide. */
#define PG_MINI_M 13          /* minimizer length for k >= 16 */
#define PG_MINI_M_SMALL 11    /* ... and for PG_MINI_MIN_K <= k <= 15 */
#define PG_MINI_MIN_K 13
#define PG_MINI_MAX_LOG2_BUCKETS 16
#define PG_MINI_MAX_ROWS ((1 << 20) - 2)
/* rows per rank of the masked count half (pg_mini_count_half_masked): a row-only record's flag rides on top of its row */
#define PG_MINI_MASKED_MAX_ROWS ((1 << 19) - 2)
#define PG_MINI_WIDE_MAX_LOG2_BUCKET_SLOTS 13
/* the bucket size of packed mini tables (k <= 21) whose caller names none, once they have 2^(PG_MINI_MAX_LOG2_BUCKETS +
 * PG_MINI_LARGE_LOG2_BUCKET_SLOTS) slots or more: buckets of 2^13 slots (64 KiB: two counting workgroups per CU) instead of the
 * largest that LDS holds, as many as PG_MINI_MAX_LOG2_BUCKETS allows -- a 2^29-slot table has 2^16 buckets of 2^13 slots, not
 * 2^15 of 2^14; smaller tables keep buckets of min(2^log2_slots, 2^PG_BUCKET_MAX_LOG2_SLOTS) slots */
#define PG_MINI_LARGE_LOG2_BUCKET_SLOTS 13
#define PG_DENSE_MAX_K 16
#define PG_HASH_MAX_K 21
#define PG_WIDE_MAX_K 31
/* pg_key42: x ^= x >> 21; x = x * M1 mod 2^42; x ^= x >> 21; x = x * M2 mod 2^42; x ^= x >> 21  (every step invertible:
 * the xorshifts are involutions on 42 bits, the multipliers are odd) */
#define PG_KEY42_M1 0x3d7ed558ccdULL
#define PG_KEY42_M2 0x1fe1a85ec53ULL
#define PG_HASH_COUNT_BITS 22
#define PG_HASH_COUNT_SAT (1u << 21)
#define PG_BUCKET_MAX_LOG2_SLOTS 14   /* 2^14 slots x 8 B = 128 KiB of the CU's 160 KiB LDS */
#define PG_BUCKET_MAX_LOG2_BUCKETS 17  /* two scatter passes of <= 9 bits; the histogram takes 2^15 bins per launch */

typedef struct {
    int32_t kind;       /* PG_TABLE_DENSE, _HASH, _WIDE or _MINI */
    int32_t k;
    int32_t log2_slots;        /* hash only */
    int32_t log2_bucket_slots; /* hash only; 0 = unbucketed */
    void *data;         /* device: uint32_t[4^k], uint64_t[2^log2_slots], or the wide form's keys followed by counts */
} pg_table;

/* Count the k-mers ending in words [word_begin, word_end) of the stream into `t`.
 * status (device uint32_t[2], zeroed by the caller): [0] is a set of PG_STATUS_* bits, non-zero after synchronising when the
 * count did not complete (PG_STATUS_TABLE_FULL: the PG_ETABLEFULL condition), [1] unused.  May be NULL for dense tables. */
#define PG_STATUS_TABLE_FULL 1u      /* a bucket (or the table) has no free slot left: enlarge log2_slots and count again */
#define PG_STATUS_OVERFLOW_LIST 2u   /* the exchange's list of count remainders >= 0xffff ran over its capacity */
#define PG_STATUS_PLAN_MISMATCH 4u   /* pg_mini_count: the plan describes more records than the record workspace holds (a plan
                                        of another stream): nothing was counted */
#define PG_STATUS_BOUNDS 8u          /* checked builds only (libpangaea_feat_checked.so): a kernel was about to store outside
                                        the buffer it was given; the store was dropped */
int pg_kmer_count(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                  const pg_table *t, uint32_t *status, void *stream);

/* HyperLogLog sketch of the distinct canonical k-mers of a word range, for sizing a table before counting:
 * registers = device uint32_t[PG_HLL_REGISTERS], zeroed by the caller (several ranges / GPUs combine by element-wise
 * max).  The registers themselves are part of the contract -- the ranks of a multi-GPU job all-reduce them with MAX:
 *   for every position of the words [word_begin, word_end) that ENDS a run of at least k characters valid under `valid`
 *   (1 <= k <= 31), with code = the canonical code of the k-mer ending there (A0 C1 T2 G3, the newest base in the low bits;
 *   complement = c ^ 2; canonical = the smaller of the forward and the reverse-complement code):
 *     h    = mix64(code ^ 0x9E3779B97F4A7C15), mix64(x): x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33;
 *            x *= 0xc4ceb9fe1a85ec53; x ^= x >> 33  (64-bit)
 *     idx  = h >> 52                                     (the top 12 bits)
 *     rank = clz64((h << 12) | (1 << 11)) + 1            (the sentinel bit below the 52 remaining hash bits: 1 <= rank <= 53)
 *     registers[idx] = max(registers[idx], rank)
 *   A k-mer belongs to the word its LAST character lies in: one that ends in word `word_begin` and starts in the word before is
 *   taken (word_begin - 1 is read), one that starts in the range and ends beyond it is not.  The call accumulates by max into
 *   whatever the registers hold, so the registers of a range are the max of those of its parts, and they depend on nothing
 *   but the SET of canonical codes.  An empty range (word_end == word_begin) launches nothing.
 * Estimate (pangaea_amd/kmer.py: sketch_estimate), m = PG_HLL_REGISTERS: E = alpha m^2 / sum_j 2^-registers[j] with
 * alpha = 0.7213 / (1 + 1.079 / m); where E <= 2.5 m and V > 0 registers are zero, m ln(m / V) instead (linear counting);
 * truncated to an integer.  tests/_sketch_ref.py restates all of this, tests/test_sketch_gpu.py holds the kernel to it. */
#define PG_HLL_REGISTERS 4096
int pg_kmer_distinct_sketch(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, int k,
                            uint32_t *registers, void *stream);

/* Rows = barcode runs that yield an output row: sorted, disjoint character ranges of the stream (device arrays). */
typedef struct {
    const int64_t *row_start; /* device [n_rows] */
    const int64_t *row_end;   /* device [n_rows] */
    int64_t n_rows;           /* < 2^22 - 1 per launch */
    /* NULL, or the STRICT validity plane (upper-case ACGT only) when the `valid` plane given to the counting call also
     * accepts lower-case bases -- jellyfish counts them (feature.py:94), the reference's own row counters reset on them
     * (count_kmer.cpp:73-78): k-mers that are only valid under the lenient rule enter the table but no row.  Device
     * uint32_t[n_words], same layout as `valid`. */
    const uint32_t *strict_valid;
} pg_rows;

/* The same result as pg_kmer_count for a bucketed hash table, without random HBM traffic: the k-mer
 * occurrences of the word range are hash-partitioned into the table's buckets by two streaming scatter
 * passes, each bucket is counted inside LDS by one workgroup and written back as its slice of the table.
 *   accumulate = 0: the table is taken to be empty and every slice is overwritten (no clearing needed);
 *   accumulate = 1: slices are loaded first, so counts add to what the table holds.
 * rows (may be NULL): when given, every partition record also carries the index of the row its k-mer ends in,
 * and the bucket-ordered records stay in the workspace for pg_abundance_from_records.
 * workspace: device scratch of pg_kmer_count_workspace_bytes(word_end - word_begin, t) bytes, 256-B aligned
 * (two record buffers of 8 B per character of the range + counters).  status as for pg_kmer_count:
 * [0] != 0 after synchronising means a bucket overflowed (PG_ETABLEFULL condition). */
int64_t pg_kmer_count_workspace_bytes(int64_t n_words, const pg_table *t);
int pg_kmer_count_bucketed(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                           const pg_table *t, int accumulate, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                           uint32_t *status, void *stream);

/* One GPU, a fresh table, abundance parameters known: pg_kmer_count_bucketed with the lookup pass of
 * pg_abundance_from_records fused into the counting kernel -- while a bucket's counts are still in LDS its records are
 * looked up and their (row, bin) words left in `shuffle_workspace` (pg_abundance_workspace_bytes); the abundance rows
 * are then finished by pg_abundance_from_emitted (same arguments as pg_abundance_from_records).  Needs rows and at least
 * 2^11 buckets. */
int pg_kmer_count_bucketed_emit(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                                const pg_table *t, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                                int window, int vsize, void *shuffle_workspace, int64_t shuffle_workspace_bytes,
                                uint32_t *status, void *stream);

/* Add n (key,count) pairs -- `pairs[i] = (pg_key42(code) << 22) | count`, the slot format -- into a hash table:
 * the merge step after tables of other GPUs have been gathered. */
int pg_kmer_merge(const uint64_t *pairs, int64_t n, const pg_table *t, uint32_t *status, void *stream);

/* (code, count) pairs into a wide table (separate arrays). */
int pg_kmer_merge_wide(const uint64_t *codes, const uint32_t *counts, int64_t n, const pg_table *t, uint32_t *status, void *stream);

/* The same merge for a bucketed table whose foreign entries arrive in bucket order (a table's slots are laid out
 * bucket by bucket, so the occupied slots of another rank's table, in slot order, already are): one workgroup per
 * bucket merges inside LDS, no global atomics.  `pairs` = n_parts vectors concatenated; seg[p * (n_buckets + 1) + b]
 * .. seg[p * (n_buckets + 1) + b + 1] delimit part p's entries of bucket b (absolute offsets into pairs, device). */
int pg_kmer_merge_bucketed(const uint64_t *pairs, const int64_t *seg, int n_parts, const pg_table *t,
                           uint32_t *status, void *stream);

/* The exchange step of the multi-GPU path in three launches around one all-gather (pangaea_amd/dist.py):
 *   pg_table_bucket_fill      fill[b] = occupied slots of bucket b (device, [n_buckets])
 *   pg_table_compact          occupied slots of bucket b -> out[seg[b] .. seg[b+1]), seg = exclusive scan of fill
 *                             (device, [n_buckets + 1]); order inside a bucket is unspecified
 *   pg_kmer_rebuild_bucketed  as pg_kmer_merge_bucketed, but the table is REBUILT from the parts alone (they include
 *                             this rank's own compacted table): the old slots are neither read nor need be initialised */
int pg_table_bucket_fill(const pg_table *t, int64_t *fill, void *stream);
/* Counting for the exchange without materialising this rank's table: `t` has the geometry of the union over all ranks
 * (the records are partitioned the way the final lookups need them), 2^group_log2 adjacent buckets are counted together
 * in one LDS table (a rank's share of the keys is that much sparser), and only the occupied entries and fill[b] are
 * produced -- t->data is NOT written.  The entries stay in the workspace until pg_deferred_gather copies bucket b's to
 * out[seg[b] ..] (seg = exclusive scan of fill).  Needs more than 256 buckets; the row-tagged records for
 * pg_abundance_from_records are left behind exactly as by pg_kmer_count_bucketed. */
#define PG_DEFERRED_MAX_GROUP_LOG2 3
int pg_kmer_count_deferred(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end,
                           const pg_table *t, int group_log2, const pg_rows *rows, void *workspace, int64_t workspace_bytes,
                           int64_t *fill, uint32_t *status, void *stream);
int pg_deferred_gather(const pg_table *t, const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                       const int64_t *fill, const int64_t *seg, uint64_t *out, void *stream);
/* The 6-byte exchange format (tables of >= 2^11 buckets): inside its bucket an entry is a 4-byte tag (the key's bits
 * below the bucket id) and a 2-byte count, sent in two planes; a count >= 0xffff sends 0xffff and its remainder as a whole
 * 8-byte entry in `overflow` (merged afterwards with pg_kmer_merge; overflow_count is a device counter, status bit 1 is set
 * when overflow_cap is too small).  tag_elem[b] / cnt_elem[b] = index of bucket b's first tag / count in the uint32 /
 * uint16 view of `out`.  pg_kmer_rebuild_planes_range rebuilds buckets [bucket_begin, bucket_end) from the gathered
 * planes: part p's tags at buf + p * part_stride_bytes, its counts 4 * cap bytes later, seg[p][j] = index of the first
 * entry of bucket bucket_begin + j (bucket_end - bucket_begin + 1 entries per part). */
int pg_deferred_gather_planes(const pg_table *t, const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                              const int64_t *fill, const int64_t *tag_elem, const int64_t *cnt_elem, void *out,
                              uint64_t *overflow, uint64_t *overflow_count, int64_t overflow_cap, uint32_t *status, void *stream);
int pg_kmer_rebuild_planes_range(const void *buf, int64_t part_stride_bytes, int64_t cap, const int64_t *seg, int n_parts,
                                 const pg_table *t, int64_t bucket_begin, int64_t bucket_end, uint32_t *status, void *stream);
/* For the owner-partitioned exchange (>= 4 ranks): a rank that has merged its own bucket range sends that range on.
 * fill[j] = occupied slots of bucket bucket_begin + j; the compaction writes the range in the 6-byte format, tag_elem /
 * cnt_elem indexed by j. */
int pg_table_bucket_fill_range(const pg_table *t, int64_t bucket_begin, int64_t bucket_end, int64_t *fill, void *stream);
int pg_table_compact_planes_range(const pg_table *t, int64_t bucket_begin, int64_t bucket_end, const int64_t *tag_elem,
                                  const int64_t *cnt_elem, void *out, uint64_t *overflow, uint64_t *overflow_count,
                                  int64_t overflow_cap, uint32_t *status, void *stream);
int pg_table_compact(const pg_table *t, const int64_t *seg, uint64_t *out, void *stream);
int pg_kmer_rebuild_bucketed(const uint64_t *pairs, const int64_t *seg, int n_parts, const pg_table *t,
                             uint32_t *status, void *stream);
/* the same for buckets [bucket_begin, bucket_end) only -- seg then has (bucket_end - bucket_begin + 1) entries per part,
 * entry j for bucket bucket_begin + j -- so that the rebuild of one range can run while the all-gather of the next is
 * still in flight */
int pg_kmer_rebuild_bucketed_range(const uint64_t *pairs, const int64_t *seg, int n_parts, const pg_table *t,
                                   int64_t bucket_begin, int64_t bucket_end, uint32_t *status, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Reading a finished table (device; one GPU, any of the five kinds; the table is only read).  The reference leaves jellyfish's
 * abundance.k{k}.count and its text dump on disk (src/feature.py:87,103) -- kept for exactly this: `jellyfish query` gives the
 * multiplicity of a k-mer, `jellyfish histo` the count spectrum from which -s and -v are chosen (how many distinct k-mers lie
 * beyond window * vector_size and so in no bin, count_kmer.cpp:86-96).  Both entries are additive to ABI 9.
 *   pg_table_query     stands in for `jellyfish query` on feature.py:87's table: counts[i] = multiplicity of codes[i], i < n
 *                      (device arrays).  A code is a k-mer in the stream's encoding (A0 C1 T2 G3, newest character in the low
 *                      bits), either strand: it is made canonical as the counting kernels do.  0: not in the table;
 *                      PG_QUERY_INVALID: the code has a bit at or above 2k (no table memory is read for it).  A wide count of
 *                      2^32 - 1 cannot be told from that.  n == 0: PG_OK, nothing launched.
 *   pg_table_spectrum  stands in for `jellyfish histo` on the same table (feature.py:87,103): hist[c] = distinct canonical
 *                      k-mers of multiplicity c for 1 <= c <= high, hist[high + 1] = those above, hist[0] = 0.  hist (device,
 *                      high + 2 words) is cleared on `stream` first and written whole.  t->data must be 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
#define PG_QUERY_INVALID 0xFFFFFFFFu
#define PG_SPECTRUM_MAX_HIGH 16382 /* high + 2 32-bit bins in 64 KiB of LDS */
int pg_table_query(const pg_table *t, const uint64_t *codes, int64_t n, uint32_t *counts, void *stream);
int pg_table_spectrum(const pg_table *t, int high, uint64_t *hist /* device, [high + 2], written whole */, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Depth of sequences in a finished table (device; one GPU, any of the five kinds; the table is only read: plain loads, no
 * atomics on it).  The sequences are character ranges of a read stream (layout at the top of this header); `valid` is the plane
 * that says what a base is, jellyfish's lenient one or the strict one.  Both entries are additive to ABI 9; every argument is
 * checked before the first HIP call.
 *   A position i HOLDS a k-mer iff i + k <= n_chars and characters i .. i + k - 1 are all set in `valid`; its COUNT is the
 *   table's multiplicity of that k-mer (made canonical as the counting kernels do), 0 if the table lacks it.  The k-mer at i
 *   BELONGS to the range [a, b) iff a <= i and i + k <= b.  Its VALUE is its count where count >= lower, else 0.
 *   pg_table_profile  stands in for `jellyfish query -s FILE` on feature.py:87's table (the multiplicity of every k-mer of a
 *                     sequence file): counts[i - char_begin] = the count at i for char_begin <= i < char_end, PG_PROFILE_NONE
 *                     where i holds no k-mer.  A wide count of 2^32 - 1 cannot be told from that.  0 <= char_begin <= char_end
 *                     <= n_chars, else PG_EINVAL; an empty range: PG_OK, nothing launched.
 *   pg_table_depth    stands beside the contig depth of scripts/bin_assembly.sh:43 (bwa + samtools +
 *                     jgi_summarize_bam_contig_depths -> contigs.megahit.depth) that scripts/low_abd_reads.sh:10 cuts at 10
 *                     and 30: a k-mer depth from a table already in device memory, the same kind of number, NOT the alignment
 *                     depth.  Per range r < n_ranges, [range_start[r], range_end[r]) (device arrays; ranges are independent:
 *                     they may overlap, repeat, be unsorted, empty, shorter than k or full of invalid characters), five
 *                     results out[r][0 .. 4] over the values of the k-mers that belong to it:
 *                       PG_DEPTH_N_KMERS  how many there are      PG_DEPTH_N_PRESENT  those with value > 0
 *                       PG_DEPTH_SUM      the sum of the values   PG_DEPTH_MAX        the largest value
 *                       PG_DEPTH_MEDIAN   the LOWER median: the value at sorted index (n_kmers - 1) / 2, zeros included
 *                     all 0 for a range without k-mers.  Preconditions 0 <= start <= end <= n_chars; whatever the device
 *                     arrays hold, bounds are clipped to [0, n_chars] and nothing outside the stream is read.  A stored count
 *                     of 2^32 - 1 (wide kinds) is taken for "no k-mer" by the long form.  Two forms, chosen per range:
 *                       short  at most PG_DEPTH_SHORT_MAX characters (reads): one wavefront per range keeps the values in
 *                              registers, selects the median there and writes the 40 bytes -- no count goes through memory;
 *                       long   anything longer (contigs, barcodes, a whole stream): the counts of its length - k + 1 positions
 *                              are stored once in the workspace, 4 bytes each, then one workgroup per range reads them for the
 *                              sums and selects the median by radix passes with a histogram in LDS.
 *                     workspace: pg_table_depth_workspace_bytes(n_long, long_positions) -- how many ranges are long and the sum
 *                     of their (length - k + 1), which the caller knows from its ranges: 256 bytes + 4 per position + 32 per
 *                     long range (at most PG_DEPTH_MAX_LONG of them in one call, else < 0); 256-byte aligned device memory,
 *                     at least pg_table_depth_workspace_bytes(0, 0) bytes (its head is cleared on `stream` by every call).  status (device uint32_t[2], zeroed by the caller): a long
 *                     range that finds no room in the workspace sets PG_STATUS_DEPTH_WORKSPACE in status[0]; the rows of the
 *                     SHORT ranges are then still right, those of the long ranges must not be used (status[0] must be 0 or
 *                     free of that bit on entry: the long form does nothing while it is set).  PG_EINVAL: a null pointer, a bad descriptor, negative sizes, lower < 1, n_ranges > 0 without
 *                     range arrays, a workspace too small or not 256-byte aligned.  n_ranges == 0: PG_OK, nothing launched.
 * ---------------------------------------------------------------------------------------------- */
#define PG_PROFILE_NONE 0xFFFFFFFFu
#define PG_DEPTH_SHORT_MAX 512 /* characters; 8 positions per lane of a wavefront, all of them in registers */
#define PG_DEPTH_MAX_LONG ((1 << 24) - 1) /* long ranges of one call: the workspace's list cursor has 24 bits */
#define PG_DEPTH_N_KMERS 0
#define PG_DEPTH_N_PRESENT 1
#define PG_DEPTH_SUM 2
#define PG_DEPTH_MAX 3
#define PG_DEPTH_MEDIAN 4
#define PG_STATUS_DEPTH_WORKSPACE 16u /* pg_table_depth: a long range found no room in the workspace: no long range's row is valid */
int pg_table_profile(const pg_table *t, const uint64_t *codes, const uint32_t *valid, int64_t n_chars, int64_t char_begin,
                     int64_t char_end, uint32_t *counts /* device, [char_end - char_begin] */, void *stream);
int64_t pg_table_depth_workspace_bytes(int64_t n_long, int64_t long_positions);
int pg_table_depth(const pg_table *t, const uint64_t *codes, const uint32_t *valid, int64_t n_chars, const int64_t *range_start,
                   const int64_t *range_end, int64_t n_ranges, int64_t lower, int64_t *out /* device, [n_ranges][5] */,
                   void *workspace, int64_t workspace_bytes, uint32_t *status, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Reads of a FASTQ text by their k-mers' counts in a finished table (device; one GPU, any of the five kinds; the table is only
 * read: plain loads, no atomics on it).  What `kmc_tools filter` and khmer's filter-abund do with a table and a read file; here
 * the alignment-free counterpart of the reference's low-abundance step, scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp, which
 * pulls the reads of low-depth contigs into *.low_abd.fq after a bwa + samtools round: the same kind of read set straight from
 * the table, and its opposite (reads made of error k-mers dropped before assembly).  The kernels work on the FASTQ TEXT in
 * device memory -- the packed read stream keeps barcode runs, not read boundaries, names or qualities.  All entries are additive
 * to ABI 9; every argument is checked before anything is enqueued (PG_EINVAL with a pg_last_error text: a null pointer, a k that
 * is not the table's, lower > upper, negative sizes, a text base that is not 16-byte aligned).
 *   INPUT    four-line FASTQ.  A line ends at '\n'; a last line without '\n' is a line; '\r' is an ordinary byte of its line
 *            (no base: a CRLF file works and is copied verbatim).  Record r is lines 4r .. 4r + 3; line 0 must begin with '@'
 *            and line 2 with '+'.  Multi-line FASTQ and FASTA are outside the contract.
 *   K-MERS   position i of the sequence line (line 1) holds a k-mer iff i + k <= its length and bytes i .. i + k - 1 are all
 *            bases: ACGT, and acgt too when lowercase_is_base; with min_qual_char = c != 0 a base whose quality byte (the same
 *            offset of line 3) is below c is no base, and a quality line shorter than its sequence line is a format error
 *            (without min_qual_char the quality line is never looked at).  The k-mer is made canonical in the table's code
 *            (A0 C1 T2 G3, (ch >> 1) & 3).
 *   HITS     n = the record's k-mers, h = those whose stored count c (0: not in the table; saturated counts as stored) satisfies
 *            lower <= c <= upper; upper < 0: no upper bound; lower >= 0 (lower = upper = 0 counts the absent k-mers).
 *   pg_fastq_index      beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its reader's getline): line_start[j] = byte
 *                       offset of line j's first byte for j < lines, line_start[lines] = n_bytes; *n_lines (device) = lines.
 *                       Entries at or beyond `cap` (>= 1) are not stored: a caller that finds *n_lines + 1 > cap calls again
 *                       with room.  workspace: pg_fastq_index_workspace_bytes(n_bytes), 8-byte aligned.  n_bytes == 0: PG_OK,
 *                       nothing launched, nothing written.
 *   pg_table_read_hits  beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its decision which read to keep, here from
 *                       k-mer counts and not from contig depth): hits[r][0] = n and hits[r][1] = h of record r < n_records of a
 *                       text whose line index holds 4 * n_records + 1 entries.  One wavefront per record, any read length.
 *                       status (device uint64_t[2], written whole by the call): [0] = PG_STATUS_FASTQ_FORMAT when a record is
 *                       malformed, else 0; [1] = PG_FASTQ_CLEAN, or ((first_record + r) << 8) | reason of the malformed record
 *                       with the SMALLEST ordinal (PG_FASTQ_NO_AT, PG_FASTQ_NO_PLUS, PG_FASTQ_SHORT_QUALITY; PG_FASTQ_BAD_INDEX:
 *                       line_start is no index of this text -- nothing outside the text is read whatever it holds).  A
 *                       malformed record's hits are 0, 0.  n_records == 0: PG_OK, nothing launched, nothing written.
 *   pg_fastq_gather     beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its writing of the chosen reads): the bytes
 *                       of record kept[i], [line_start[4 r], line_start[4 r + 4]), go to out + dst_off[i] for i < n_kept, byte
 *                       for byte (a final record without its '\n' leaves without one).  dst_off is the caller's exclusive scan
 *                       of the kept records' lengths.  One wavefront per kept record; nothing outside [0, n_bytes) of the text
 *                       is read and nothing outside [0, out_bytes) of out written, whatever the device arrays hold.
 *                       n_kept == 0: PG_OK, nothing launched.
 * Which records are kept -- the pass rule (n >= 1, min_hits <= h <= max_hits, absolute or as a share of n) and the pair rule
 * (any / both / single) -- is the caller's: a few element-wise operations on [n_records] arrays (pangaea_amd/kmer.py,
 * KmerTable.filter_fastq).
 * ---------------------------------------------------------------------------------------------- */
#define PG_STATUS_FASTQ_FORMAT 32u /* pg_table_read_hits: a record of the text is malformed; status[1] says which and why */
#define PG_FASTQ_CLEAN 0xFFFFFFFFFFFFFFFFull
#define PG_FASTQ_NO_AT 1u
#define PG_FASTQ_NO_PLUS 2u
#define PG_FASTQ_SHORT_QUALITY 3u
#define PG_FASTQ_BAD_INDEX 4u
int64_t pg_fastq_index_workspace_bytes(int64_t n_bytes);
int pg_fastq_index(const uint8_t *text, int64_t n_bytes, int64_t *line_start /* device, [cap] */, int64_t cap,
                   int64_t *n_lines /* device [1] */, void *workspace, int64_t workspace_bytes, void *stream);
int pg_table_read_hits(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                       int64_t first_record, int64_t lower, int64_t upper /* < 0: none */, int lowercase_is_base,
                       int min_qual_char /* 0: none */, uint32_t *hits /* device, [n_records][2] */,
                       uint64_t *status /* device [2] */, void *stream);
int pg_fastq_gather(const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records, const int64_t *kept,
                    const int64_t *dst_off, int64_t n_kept, uint8_t *out, int64_t out_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Reads of a FASTQ text trimmed to their solid span (device; one GPU, any of the five kinds; the table is only read).  The second
 * mode of the tools the section above is modelled on -- `kmc_tools filter -t`, khmer's filter-abund / trim-low-abund: a read
 * is cut down to the part the table vouches for and not dropped, so that a read with one sequencing error keeps its good
 * bases.  Beside the same step of the reference, scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp.  INPUT, K-MERS, the count
 * window lower <= c <= upper, lowercase_is_base and min_qual_char are exactly those of pg_table_read_hits.  Both entries are
 * additive to ABI 9; every argument is checked before the first HIP call (PG_EINVAL with a pg_last_error text: a null pointer
 * by name, a k that is not the table's, lower > upper, negative sizes, a mode that is none, a text base that is not 16-byte
 * aligned, n_kept outside [0, n_records]).
 *   SOLID    position i of a sequence line is solid iff it holds a k-mer and that k-mer's stored count is inside the window.  A
 *            position that holds no k-mer -- an 'N', a '\r', a masked base among its k bytes, or i + k > length -- is not solid.
 *   RUN      a maximal interval [a, b) of solid positions; its SPAN is the bases [a, b + k - 1): start a, length b - a + k - 1.
 *   MODE     PG_SPAN_FIRST: the run that begins at position 0 (`kmc_tools filter -t` / khmer: cut at the first k-mer outside
 *            the window); the empty span (0, 0) if position 0 is not solid.  PG_SPAN_LONGEST: the longest run, among equals
 *            the leftmost; (0, 0) if the record has no solid position.
 *   N, H     those of pg_table_read_hits, over the whole line in both modes (FIRST takes no early exit: one pass gives hits and
 *            span, and the totals stay exact).
 *   CR       cr_s = 1 iff the sequence line is non-empty and its last byte is '\r'; cr_q the same for the quality line's
 *            content (the line without its '\n').
 *   TRIMMED  the record cut to its span (start, length): line 0 verbatim with its newline; seq[start : start + length], '\r'
 *            if cr_s, '\n'; line 2 verbatim; qual[start : start + length], '\r' if cr_q, '\n' iff the record ended in one.
 *            Quality bytes beyond the sequence's length are dropped: the output is always a well-formed record.
 *   SHORT    qual_len - cr_q < seq_len - cr_s is malformed (PG_FASTQ_SHORT_QUALITY) ALWAYS here, not only under min_qual_char:
 *            the quality line is cut too.  (Under min_qual_char the rule of pg_table_read_hits holds as well.)
 *   pg_table_read_spans      beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its decision which read to keep; here which
 *                            part of it): spans[r] = n, h, start, length of record r < n_records and trimmed_bytes[r] = the bytes
 *                            of its trimmed record, (s1 - s0) + length + cr_s + 1 + (s3 - s2) + length + cr_q + nl with s0 .. s3
 *                            its four line starts and nl = 1 iff it ends in '\n'.  One wavefront per record, any read length;
 *                            status as pg_table_read_hits writes it (the same two words, the same reasons).  A malformed
 *                            record's row is 0, 0, 0, 0 and its trimmed_bytes 0.  n_records == 0: PG_OK, nothing launched,
 *                            nothing written.
 *   pg_fastq_gather_trimmed  beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its writing of the chosen reads): the
 *                            trimmed record of r = kept[i], span spans[r][2], spans[r][3], goes to out + dst_off[i] for
 *                            i < n_kept; dst_off is the caller's exclusive scan of trimmed_bytes over the kept records.  One
 *                            wavefront per kept record.  cr_s, cr_q, nl are read from the text again and everything handed in
 *                            is checked: a record is skipped when r is out of range, its index is not monotone inside the
 *                            text, start + length exceeds the sequence's or the quality's bases, or its bytes do not fit
 *                            [dst_off[i], out_bytes).  Nothing outside [0, n_bytes) of the text is read and nothing outside
 *                            [0, out_bytes) of out written.  n_kept == 0: PG_OK, nothing launched.
 * Which records are written -- span length >= min_len, the pair rule -- is the caller's (KmerTable.trim_fastq).
 * ---------------------------------------------------------------------------------------------- */
#define PG_SPAN_FIRST 0
#define PG_SPAN_LONGEST 1
int pg_table_read_spans(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                        int64_t first_record, int64_t lower, int64_t upper /* < 0: none */, int lowercase_is_base,
                        int min_qual_char /* 0: none */, int mode,
                        uint32_t *spans /* device, [n_records][4]: n, h, start, length */,
                        int64_t *trimmed_bytes /* device, [n_records] */, uint64_t *status /* device [2] */, void *stream);
int pg_fastq_gather_trimmed(const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                            const int64_t *kept, const uint32_t *spans /* [n_records][4] */, const int64_t *dst_off,
                            int64_t n_kept, uint8_t *out, int64_t out_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Single substitutions in the reads of a FASTQ text put right (device; one GPU, any of the five kinds; the table is only read).
 * The third mode of the tools the two sections above are modelled on -- khmer, Lighter, BFC, Musket, beside `kmc_tools filter`:
 * a read is neither dropped nor cut, the wrong base is replaced.  Beside the same step of the reference,
 * scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp.  INPUT, K-MERS, the count window lower <= c <= upper, lowercase_is_base
 * and min_qual_char are exactly those of pg_table_read_hits, SHORT is the rule of pg_table_read_spans (a quality line that does
 * not reach as far as its sequence line is malformed always).  The entry is additive to ABI 9; every argument is checked
 * before the first HIP call (PG_EINVAL with a pg_last_error text: a null pointer by name, a k that is not the table's,
 * lower > upper, negative sizes, a min_qual_char that is no byte, a text base that is not 16-byte aligned).
 *   BASES      of a sequence line: its bytes without a final '\r' (cr_s of the section above).  len is their number and
 *              n_pos = max(0, len - k + 1).  The '\r' is beyond the end here, not a position without a k-mer, so that the
 *              right-end errors of CRLF files are corrected too.
 *   CLASS      of position i < n_pos: S (solid) -- it holds a k-mer whose stored count is inside the window; W (weak) -- it
 *              holds a k-mer whose count is outside the window (absent: 0); V (void) -- it holds no k-mer: an 'N', a masked or
 *              a low-quality base is among its k bytes.  Positions -1 and n_pos are E (the end).
 *   CANDIDATE  a maximal run [a, b) of W positions whose neighbours a - 1 and b are both in {S, E} and not both E, of one of
 *              these shapes, with the base p in question:
 *                  left S, right S, b - a == k:   p = b - 1  (= a + k - 1)
 *                  left E, right S, b - a <= k:   p = b - 1
 *                  left S, right E, b - a <= k:   p = a + k - 1
 *              This is what one substitution at base p does to the flags when no erroneous k-mer is solid by chance: every
 *              k-mer at a position of [a, b) contains base p and no other k-mer does.  No candidates: a run with a V
 *              neighbour, an interior run of any other length (two errors d < k apart give k + d), an all-weak read.
 *   REPAIR     for each of the three bases x of A, C, G, T other than the base at p (compared without regard to case under
 *              lowercase_is_base): x is VALID iff all b - a k-mers at [a, b), read with x at p, have a stored count inside
 *              the same window.  The candidate is CORRECTED iff exactly one x is valid: byte p of the sequence line becomes
 *              that x in the letter case of the byte it replaces.  With no valid x, or two or three, the byte stays.  The
 *              quality line is never changed.
 *   ONE PASS   all candidates of a record are judged on the record as it came; they do not interact (a k-mer contains at most
 *              one p).  After the pass h has grown by exactly the sum of b - a over the corrected runs, and a second pass over
 *              the output finds candidates - corrected candidates and corrects none.
 *   ROW        n, h, candidates, corrected of record r < n_records; n and h are those of pg_table_read_hits on the input.  A
 *              malformed record gives 0, 0, 0, 0 and the status words as pg_table_read_hits writes them.
 *   pg_table_correct_reads   beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its decision about a read; here the
 *                            repair of one).  One wavefront per record, any read length, any number of candidates.  out:
 *                            NULL -- rows only; a device buffer of n_bytes into which the caller has copied text; or text
 *                            itself -- in place.  The kernel stores nothing but the corrected bytes out[s1 + p] (s1: the
 *                            start of the record's sequence line) and the rows: no byte outside [0, n_bytes) of the text is
 *                            read and none outside the record's sequence line written, whatever the index says.
 *                            n_records == 0: PG_OK, nothing launched, nothing written.
 * ---------------------------------------------------------------------------------------------- */
int pg_table_correct_reads(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                           int64_t first_record, int64_t lower, int64_t upper /* < 0: none */, int lowercase_is_base,
                           int min_qual_char /* 0: none */, uint8_t *out /* device: NULL, a copy of text, or text */,
                           uint32_t *rows /* device, [n_records][4]: n, h, candidates, corrected */, uint64_t *status /* device [2] */,
                           void *stream);

/* ----------------------------------------------------------------------------------------------
 * Depth of the reads of a FASTQ text (device; one GPU, any of the five kinds; the table is only read).  What BBNorm and khmer's
 * normalize-by-median decide a read's fate by: the median -- here any percentile -- of the counts of its k-mers, and beside it
 * a reproducible draw per read or pair, so that the caller can keep a read with probability target / depth.  Beside the same
 * step of the reference, scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp.  INPUT, K-MERS, lowercase_is_base, min_qual_char
 * and the status words are exactly those of pg_table_read_hits.  The entry is additive to ABI 9; every argument is checked
 * before the first HIP call (PG_EINVAL with a pg_last_error text: a null pointer by name, a k that is not the table's,
 * lower < 1, a percentile outside [0, 100], a unit_log2 that is neither 0 nor 1, negative sizes, a min_qual_char that is no
 * byte, a text or rows base that is not 16-byte aligned).
 *   VALUE    of a k-mer: its stored count c (0: absent; saturated counts as stored), taken as 0 when c < lower.
 *   ROW      n, present, d, w of record r < n_records: n = the k-mers of the record, present = its values > 0, d = the value
 *            at index ((n - 1) * percentile) / 100 (integer division) of the n values in ascending order, 0 when n = 0 --
 *            percentile 50 is the lower median of pg_table_depth --, w = the draw of the record's unit.  A malformed record
 *            gives 0, 0, 0, 0 and the status words as pg_table_read_hits writes them.
 *   DRAW     of unit u = (first_record + r) >> unit_log2 (0: every record is a unit; 1: records 2i and 2i + 1 of an
 *            interleaved file share one), in arithmetic mod 2^64 -- splitmix64 of seed + (u + 1) * its increment, top 24 bits:
 *                z = seed + (u + 1) * 0x9E3779B97F4A7C15;   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *                z = (z ^ (z >> 27)) * 0x94D049BB133111EB;   z ^= z >> 31;   w = z >> 40
 *            w depends on nothing but seed and the record's ordinal: pieces of any size give the same draws.  A caller that
 *            keeps a read iff w * d < target * 2^24 (exact in 64 bits: w < 2^24, d < 2^32) keeps it with probability
 *            min(1, target / d).
 *   pg_table_read_depths   beside scripts/low_abd_reads.sh:10 / extract_unmapped.cpp (its decision which read to keep, here from
 *                          the depth the table gives the read).  One wavefront per record and any read length, with no
 *                          workspace: a record of at most 512 positions keeps its values in registers and finds d by a search
 *                          over the bits of the value; a longer one takes one sweep for n, present and the maximum and one per
 *                          8-bit digit of d, each looking its k-mers up again (at most 1 + 4 sweeps).  Each row leaves as one
 *                          16-byte store.  n_records == 0: PG_OK, nothing launched, nothing written.
 * ---------------------------------------------------------------------------------------------- */
int pg_table_read_depths(const pg_table *t, int k, const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_records,
                         int64_t first_record, int64_t lower /* >= 1 */, int percentile /* 0 .. 100 */, int lowercase_is_base,
                         int min_qual_char /* 0: none */, uint64_t seed, int unit_log2 /* 0 or 1 */,
                         uint32_t *rows /* device, 16-byte aligned, [n_records][4]: n, present, d, w */, uint64_t *status /* device [2] */,
                         void *stream);

/* ----------------------------------------------------------------------------------------------
 * Read pairs of a FASTQ text by their barcode tag (device; one GPU; no table).  Every entry point of this library takes a
 * barcode-sorted interleaved FASTQ; the reference makes one in step 0 of its driver, src/run_pangaea:237-252: an awk pass glues
 * each 8-line block to the BX:Z: tag of its first header, then `LANG=C sort -k1,1 | cut | tr`.  These entries are what that step
 * needs to know about the barcode ON THE TEXT in device memory; the line index is pg_fastq_index's and the records are moved
 * by pg_fastq_gather (pangaea_amd/sortreads.py: sort_fastq, check_fastq).  All entries are additive to ABI 9; every argument is
 * checked before the first HIP call (PG_EINVAL with a pg_last_error text: a null pointer by name, negative sizes, a
 * lines_per_unit that is neither 4 nor 8, a byte_begin that is negative or no multiple of 8, a text base that is not 16-byte
 * aligned).  Whatever the device arrays hold, nothing outside [0, n_bytes) of the text is read and nothing outside the output
 * arrays written; text and arrays go through plain loads and stores.
 *   UNIT     a read pair: lines_per_unit = 8 lines of an interleaved four-line FASTQ, or lines_per_unit = 4: one record of an
 *            R1 file (its mate is the same record of R2, which these entries never see).  The header of unit u is line
 *            lines_per_unit * u of a line index of lines_per_unit * n_units + 1 entries.
 *   TAG      taken from that header only -- a tag on the mate's header is ignored: the LEFTMOST match of "BX:Z:" followed by one
 *            or more bytes that are no C-locale white space (space, \t, \n, \v, \f, \r), at its longest.  "BX:Z:" right in
 *            front of white space or of the line's end is no match there; a later occurrence in the line can still match.
 *            '\r' ends a tag (CRLF files).  A unit without a match is UNTAGGED.  NUL bytes in a header are outside the contract.
 *   ORDER    tagged units first, by the bytes of their tags as unsigned bytes, of two tags of which one is a prefix of the
 *            other the shorter first (memcmp, then length: `LANG=C sort -k1,1` on a key without blanks); untagged units behind
 *            all tagged ones (the reference gives them the key "~~~"; every tag begins with 'B') and equal to each other.
 *            WITHIN one tag the reference's order is GNU sort's last-resort comparison of the whole line (read name, then
 *            sequence); callers of these entries keep the INPUT order instead (a stable sort): nothing downstream reads that
 *            order, and a stable order is reproducible and cheaper.
 *   pg_fastq_barcode_tags  beside src/run_pangaea:237-252 (awk's match(): which bytes are the tag): tag_off[u] = byte offset of
 *                          the 'B' of the match or -1, tag_len[u] = length of the whole match ("BX:Z:" included) or 0, u <
 *                          n_units.  status (device uint64_t[2], written whole by the call) as pg_table_read_hits writes it:
 *                          [0] = PG_STATUS_FASTQ_FORMAT or 0, [1] = PG_FASTQ_CLEAN or (record << 8) | reason of the malformed
 *                          record with the smallest ordinal, record = u * (lines_per_unit / 4) + (0: R1's, 1: R2's) --
 *                          PG_FASTQ_NO_AT, PG_FASTQ_NO_PLUS and PG_FASTQ_BAD_INDEX for every record of the unit,
 *                          PG_FASTQ_LONG_TAG for a tag of more than PG_FASTQ_MAX_TAG bytes behind "BX:Z:" (reported on the
 *                          unit's first record).  A malformed unit leaves as untagged (-1, 0).  One wavefront per header, 64
 *                          bytes per turn, any header length.  n_units == 0: PG_OK, nothing launched, nothing written.
 *   pg_fastq_tag_keys      beside src/run_pangaea:237-252 (the key bytes `sort -k1,1` compares): keys[i] = bytes [byte_begin,
 *                          byte_begin + 8) of the tag of unit order[i] (order NULL: unit i) counted BEHIND the 5-byte prefix,
 *                          big-endian -- the first byte highest -- and zero behind the tag's end, i < n; 0 for an untagged unit
 *                          and for an order[i] outside [0, n).  tag_off, tag_len: n entries, as the entry above wrote them
 *                          (anything else reads as untagged).  Compared as UNSIGNED words, chunk after chunk, the keys give
 *                          the order of the tagged units; untagged units must be told by tag_len, not by a key (eight 0xFF
 *                          bytes are a legal tag).  n == 0: PG_OK, nothing launched.
 *   pg_fastq_tag_compare   beside src/run_pangaea:237-252 (sort's comparison itself): out[0] = 0, out[i] = -1, 0 or +1 as
 *                          tag(order[i - 1]) stands before, equal to or behind tag(order[i]) in ORDER, i < n (order NULL:
 *                          identity).  Never goes through a key: the independent statement of the order.  On the identity any +1
 *                          is a descent (the file is not sorted); on a sorted order the number of -1 plus one is the number of
 *                          runs.  n == 0: PG_OK, nothing launched.
 * ---------------------------------------------------------------------------------------------- */
#define PG_FASTQ_LONG_TAG 5u   /* beside PG_FASTQ_NO_AT .. PG_FASTQ_BAD_INDEX: a tag longer than PG_FASTQ_MAX_TAG */
#define PG_FASTQ_MAX_TAG 255   /* bytes of a tag behind "BX:Z:" */
int pg_fastq_barcode_tags(const uint8_t *text, int64_t n_bytes, const int64_t *line_start, int64_t n_units, int lines_per_unit /* 4 or 8 */,
                          int64_t *tag_off /* device, [n_units] */, int32_t *tag_len /* device, [n_units] */,
                          uint64_t *status /* device [2] */, void *stream);
int pg_fastq_tag_keys(const uint8_t *text, int64_t n_bytes, const int64_t *tag_off, const int32_t *tag_len,
                      const int64_t *order /* device, [n], or NULL */, int64_t n, int64_t byte_begin, uint64_t *keys /* device, [n] */,
                      void *stream);
int pg_fastq_tag_compare(const uint8_t *text, int64_t n_bytes, const int64_t *tag_off, const int32_t *tag_len,
                         const int64_t *order /* device, [n], or NULL */, int64_t n, int8_t *out /* device, [n] */, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Raw stLFR and TELL-seq read pairs brought to the BX:Z: form (device; one GPU; no table).  The section above sorts reads whose
 * barcode stands in a BX:Z: tag; the reference's driver makes that form first -- the other half of its step 0 -- with
 * `preprocess_stlfr -n -l` (src/run_pangaea:138-149 -> preprocess_stlfr.cpp:68-113) and `preprocess_tellseq -l INDEX`
 * (src/run_pangaea:151-162 -> preprocess_tellseq.cpp:52-84), then `seqtk mergepe` (src/run_pangaea:224).  These entries do the
 * same rewriting ON THE TEXTS in device memory (pangaea_amd/prepreads.py: preprocess_reads; sortreads.py with short_type).
 * Both are additive to ABI 9; every argument is checked before the first HIP call (PG_EINVAL with a pg_last_error text: a
 * mode that is none, a null pointer by name, negative sizes, a text base that is not 16-byte aligned, an index text without
 * PG_PREP_TELLSEQ, n_kept outside [0, n_units]).  Whatever the device arrays hold, nothing outside [0, n_bytes) of a text is read
 * and nothing outside [0, out_bytes) of an output written; plain loads and stores.  These are BYTE rules: a line's content is
 * the line without its '\n', a '\r' is an ordinary byte of the content.  The reference checks nothing (it writes garbage or
 * aborts on malformed input): parity is claimed on well-formed input only.
 *   UNIT      record u of R1 (text1) with record u of R2 (text2) and, for TELL-seq, of I1 (text_i), each four lines of a line
 *             index of 4 * n_units + 1 entries.  h = the content of R1's header.
 *   STLFR     (PG_PREP_STLFR; preprocess_stlfr.cpp:68-113 with -n -l)  p = the first '#' in h (none: PG_FASTQ_NO_HASH); q = the
 *             first '/' behind p, or the end of h; B = h[p + 1 : q].  B is split at its first two '_' into f1, f2 and the rest
 *             f3, which may hold more '_' (fewer than two '_': PG_FASTQ_FEW_FIELDS -- the reference aborts on .at()); B of more
 *             than PG_FASTQ_MAX_TAG - 2 bytes: PG_FASTQ_LONG_TAG, so that the tag with its "-1" still fits the sort's limit.
 *             The unit is TAGGED iff f1 != "0" and f2 != "0", compared as byte strings.  The reference tests f1 twice and never
 *             f3 (preprocess_stlfr.cpp:89): 5_6_0 is tagged, 5_0_7, 0_6_7 and 0_0_0 are not -- kept exactly so.  The new header
 *             of BOTH mates is h[:p], then "\tBX:Z:" + B + "-1" if tagged, then '\n': R2's own header is discarded (only its '@'
 *             is checked).  Lines 1, 2 and 3 of each mate are copied byte for byte.  No unit is dropped.
 *   TELLSEQ   (PG_PREP_TELLSEQ; preprocess_tellseq.cpp:52-84)  B = the content of the SEQUENCE line of I1's record u.  The unit
 *             is KEPT iff B has exactly 18 bytes (a B with a trailing '\r' has 19 and is dropped, as the reference drops it; no
 *             error).  s = the first space (0x20) in h, or the end of h -- a tab does not cut.  The new header of both mates is
 *             h[:s] + "\tBX:Z:" + B + "-1" + '\n'; line 1 is copied byte for byte, line 2 becomes exactly "+\n" whatever it
 *             held, line 3 is copied byte for byte.  The white list (PREFIX.wl) is B + '\n' per kept unit, in input order.
 *   BOTH      a last line without '\n' gets one.  Malformed: a header without '@' (PG_FASTQ_NO_AT) or a third line without '+'
 *             (PG_FASTQ_NO_PLUS) in ANY of the two or three files, PG_FASTQ_BAD_INDEX, and the three stLFR reasons above.  A
 *             file that ends inside a record and files of different record counts are the caller's to refuse (they show in
 *             the line counts).
 *   pg_fastq_prep_plan   beside preprocess_stlfr.cpp:76-91 / preprocess_tellseq.cpp:62-72 (where the barcode lies and whether
 *                        the unit is tagged / kept): head_len[u] = p resp. s counted from the header's first byte; bc_off[u] =
 *                        byte offset of B in text1 (stLFR) resp. text_i (TELL-seq), bc_len[u] = its bytes; tagged[u] = 1 for a
 *                        tagged (stLFR) resp. kept (TELL-seq) unit, else 0.  A malformed unit leaves 0, -1, 0, 0.  status
 *                        (device uint64_t[3][2], written whole by the call): row f for file f (0 R1, 1 R2, 2 I1) as
 *                        pg_table_read_hits writes its two words -- [0] = PG_STATUS_FASTQ_FORMAT or 0, [1] = PG_FASTQ_CLEAN or
 *                        ((first_unit + u) << 8) | reason of the malformed record with the SMALLEST ordinal in that file; the
 *                        stLFR reasons stand in row 0.  One wavefront per unit, 64 header bytes per turn, any header length.
 *                        n_units == 0: PG_OK, nothing launched, nothing written.
 *   pg_fastq_prep_write  beside preprocess_stlfr.cpp:92-108 / preprocess_tellseq.cpp:63-79 (the writing): for i < n_kept and
 *                        u = kept[i] (kept NULL: u = i) the new record of R1 goes to out1 + dst1[i] and that of R2 to out2 +
 *                        dst2[i].  Its bytes: head_len[u] + (tagged[u] ? 8 + bc_len[u] : 0) + 1, then stLFR: the bytes of lines
 *                        1 .. 3, TELL-seq: those of line 1, 2, those of line 3; + 1 when the record lacks its final '\n'.  dst1 /
 *                        dst2 are the caller's exclusive scans of these.  out1 and out2 may be ONE buffer: with dst2[i] =
 *                        dst1[i] + (bytes of R1's new record) that is the interleaved form `seqtk mergepe` makes.  The plan
 *                        arrays are checked again: a unit is skipped when u is out of range, an index is not monotone inside
 *                        its text, head_len exceeds the header, B does not lie inside its text or is longer than
 *                        PG_FASTQ_MAX_TAG - 2, a TELL-seq unit is not tagged, or a record does not fit [dst, out_bytes).  One
 *                        wavefront per kept unit.  white_list (TELL-seq only, or NULL): B + '\n' of kept unit i at 19 i,
 *                        inside [0, white_list_bytes).  n_kept == 0: PG_OK, nothing launched.
 * ---------------------------------------------------------------------------------------------- */
#define PG_FASTQ_NO_HASH 6u     /* beside PG_FASTQ_NO_AT .. PG_FASTQ_LONG_TAG: a stLFR header without '#' */
#define PG_FASTQ_FEW_FIELDS 7u  /* a stLFR barcode with fewer than two '_' */
#define PG_PREP_STLFR 1
#define PG_PREP_TELLSEQ 2
int pg_fastq_prep_plan(int mode, const uint8_t *text1, int64_t n1_bytes, const int64_t *line_start1, const uint8_t *text2, int64_t n2_bytes,
                       const int64_t *line_start2, const uint8_t *text_i /* PG_PREP_TELLSEQ, else NULL */, int64_t n_i_bytes,
                       const int64_t *line_start_i, int64_t n_units, int64_t first_unit, int64_t *head_len /* device, [n_units] */,
                       int64_t *bc_off /* device, [n_units] */, int32_t *bc_len /* device, [n_units] */,
                       uint8_t *tagged /* device, [n_units] */, uint64_t *status /* device [3][2] */, void *stream);
int pg_fastq_prep_write(int mode, const uint8_t *text1, int64_t n1_bytes, const int64_t *line_start1, const uint8_t *text2, int64_t n2_bytes,
                        const int64_t *line_start2, const uint8_t *text_i /* PG_PREP_TELLSEQ, else NULL */, int64_t n_i_bytes,
                        int64_t n_units, const int64_t *head_len, const int64_t *bc_off, const int32_t *bc_len, const uint8_t *tagged,
                        const int64_t *kept /* device, [n_kept], or NULL */, const int64_t *dst1, const int64_t *dst2, int64_t n_kept,
                        uint8_t *out1, int64_t out1_bytes, uint8_t *out2, int64_t out2_bytes,
                        uint8_t *white_list /* PG_PREP_TELLSEQ, or NULL */, int64_t white_list_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * The table as jellyfish's text dump, and back (device; one GPU, any of the five kinds).  The reference keeps
 * abundance.k{k}.dump on disk (src/feature.py:87,103: `jellyfish dump -c -t`), count_kmer -g reads it (count_kmer.cpp:139-170).
 * One line per entry, "<k-mer>\t<count>\n": the first character from the highest two bits of the canonical code, A C T G for
 * 0 1 2 3; the count is the stored value (packed kinds stop at PG_HASH_COUNT_SAT).  Lines stand in slot order, so the text of a
 * table is one fixed byte string and can be written range by range.  All entries are additive to ABI 9; every argument is
 * checked before the first HIP call; the table is only read (plain loads) and t->data must be 16-byte aligned.
 *   pg_table_dump_units  the table's units: PG_DUMP_UNIT_SLOTS consecutive entries each (the last may be short: 4^k < a unit)
 *   pg_table_dump_sizes  stands in for the sizing of `jellyfish dump -c -t -L lower` (feature.py:87,103): unit_bytes[u] = text
 *                        bytes of unit u, k + 2 + digits(count) per entry with count >= lower (lower >= 1; 1 = every entry);
 *                        unit_lines[u] (may be NULL) = its lines.  Device arrays of pg_table_dump_units(t) words.
 *   pg_table_dump_text   stands in for `jellyfish dump -c -t -L lower` itself (feature.py:87,103): the lines of units
 *                        [unit_begin, unit_end) go to text + (unit_offsets[u] - text_base), unit_offsets (device) being the
 *                        exclusive scan of unit_bytes.  text_base and range_bytes are what the caller knows of that scan on the
 *                        host: unit_offsets[unit_begin] and unit_offsets[unit_end] - unit_offsets[unit_begin]; a text buffer
 *                        shorter than range_bytes is refused, and whatever the device offsets say, no byte outside
 *                        [0, range_bytes) of text is written.  An empty range or range_bytes == 0: PG_OK, nothing launched.
 *   pg_dump_parse        stands in for the dump reload of count_kmer.cpp:139-170 over n_bytes of text (device, 16-byte aligned)
 *                        that hold whole lines; a last line without newline is a line.  Per line: the text before the first
 *                        TAB must have exactly k characters (else PG_DUMP_BAD_LENGTH; a line without TAB: PG_DUMP_NO_TAB); the
 *                        count is the 1 to PG_DUMP_MAX_DIGITS decimal digits behind the TAB, followed by the end of the line,
 *                        one '\r' before it tolerated (else PG_DUMP_BAD_COUNT); blank lines are skipped; a k-mer with a character
 *                        outside ACGT (N, lower case) is dropped silently, as count_kmer.cpp:153 drops it.  Kept lines leave as
 *                        codes[i] (canonical, (c >> 1) & 3 per character), counts[i], ordinals[i] = first_ordinal + the line's
 *                        0-based index in the text, i < n_out[0], in no particular order (later lines override earlier ones,
 *                        count_kmer.cpp:166: the caller's business, by ordinal); n_out[1] = lines of the text, blank ones
 *                        included.  status (device, one word): PG_DUMP_CLEAN, or (1-based line << 8) | reason of the FIRST bad
 *                        line (PG_DUMP_CAPACITY: more kept lines than cap) -- the output of such a call must not be used.
 *                        workspace: pg_dump_parse_workspace_bytes(n_bytes), 8-byte aligned.  n_bytes == 0: PG_OK, nothing
 *                        launched, nothing written.
 * ---------------------------------------------------------------------------------------------- */
#define PG_DUMP_UNIT_SLOTS 1024 /* one workgroup of 256 lanes x 4 entries; its text (<= 43 bytes per line) fits 44 KiB of LDS */
#define PG_DUMP_MAX_DIGITS 18
#define PG_DUMP_CLEAN 0xFFFFFFFFFFFFFFFFull
#define PG_DUMP_BAD_LENGTH 1u
#define PG_DUMP_NO_TAB 2u
#define PG_DUMP_BAD_COUNT 3u
#define PG_DUMP_CAPACITY 4u
int64_t pg_table_dump_units(const pg_table *t);
int pg_table_dump_sizes(const pg_table *t, int64_t lower, int64_t *unit_bytes, int64_t *unit_lines /* may be NULL */, void *stream);
int pg_table_dump_text(const pg_table *t, int64_t lower, int64_t unit_begin, int64_t unit_end, const int64_t *unit_offsets,
                       int64_t text_base, int64_t range_bytes, uint8_t *text, int64_t text_bytes, void *stream);
int64_t pg_dump_parse_workspace_bytes(int64_t n_bytes);
int pg_dump_parse(const uint8_t *text, int64_t n_bytes, int k, int64_t first_ordinal, uint64_t *codes, uint64_t *counts,
                  int64_t *ordinals, int64_t cap, int64_t *n_out /* device [2] */, uint64_t *status /* device [1] */,
                  void *workspace, int64_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Merging finished tables (device; one GPU, any of the five kinds).  The reference counts every read of a sample into ONE
 * jellyfish table (src/feature.py:76-94); a sample that arrives as several files -- lanes, runs, a dump from elsewhere plus new
 * reads -- becomes that table through `jellyfish merge`: one table that holds the sum of several.  All three entries are additive
 * to ABI 9; every argument is checked before anything is enqueued (PG_EINVAL with a pg_last_error text: a null pointer, differing
 * k, a kind that does not admit k, differing geometry for the aligned form, dst overlapping a source, n_srcs outside 1..16);
 * sources are only read (plain loads), every t->data must be 16-byte aligned.  Sums of 2^32 and more are outside the contract,
 * as they are for counting.
 *   pg_table_merge          replaces `jellyfish merge` over the tables of feature.py:76-94, general form: every entry of `src`
 *                           is ADDED to what `dst` holds, whatever the two kinds and geometries (both must admit the same k).
 *                           Dense: atomic adds; hash / mini: counts saturate at PG_HASH_COUNT_SAT exactly (a packed source's
 *                           saturated count travels as the value it stores, 2^21); wide / wide mini: 32-bit sums.  A
 *                           destination without room sets PG_STATUS_TABLE_FULL in status[0] (device uint32_t[2], zeroed by the
 *                           caller; may be NULL for a dense dst): enlarge it and merge again.
 *   pg_table_merge_aligned  replaces `jellyfish merge` over the tables of feature.py:76-94 where dst and the n_srcs sources
 *                           (1..16; the same source may appear twice) are all PG_TABLE_MINI, or all PG_TABLE_HASH in buckets of
 *                           at most 2^PG_BUCKET_MAX_LOG2_SLOTS slots, with one k, log2_slots and log2_bucket_slots: a k-mer
 *                           then lies in the same bucket of every table, one workgroup per bucket sums the sources' slices
 *                           inside LDS and writes the slice of dst once -- only streams, no global atomics.  dst is REBUILT:
 *                           its old content is neither read nor need be initialised.  A bucket whose union does not fit sets
 *                           PG_STATUS_TABLE_FULL (dst is then incomplete: take pg_table_merge into a larger table).
 *   pg_table_merge_aligned_applies  replaces nothing of the reference: the one statement of the rule above -- 1 when tables a
 *                           and b (kinds, k and geometry, their data is not looked at) may stand together in a
 *                           pg_table_merge_aligned call (`jellyfish merge` over the tables of feature.py:76-94), else 0.
 * ---------------------------------------------------------------------------------------------- */
int pg_table_merge(const pg_table *dst, const pg_table *src, uint32_t *status, void *stream);
int pg_table_merge_aligned(const pg_table *dst, const pg_table *const *srcs, int n_srcs, uint32_t *status, void *stream);
int pg_table_merge_aligned_applies(const pg_table *a, const pg_table *b);

/* ----------------------------------------------------------------------------------------------
 * Combining finished tables otherwise than by their sum (device; one GPU, any of the five kinds).  The tables are those of
 * src/feature.py:76-94 and the dump count_kmer.cpp:139-170 reads; the reference itself never combines two of them, so these
 * entries stand beside those lines and replace nothing of the reference.  For a canonical k-mer let a be the count table `a`
 * STORES for it and b the count table `b` stores, 0 where absent (a packed kind stops at PG_HASH_COUNT_SAT: the stored value
 * counts, as in pg_table_merge).  The result holds r, and only where lower <= r <= upper (lower >= 1; upper < 0: no upper bound):
 *   PG_COMBINE_MIN   min(a, b)              intersection, the smaller count
 *   PG_COMBINE_MAX   max(a, b)              union, the larger count
 *   PG_COMBINE_DIFF  a > b ? a - b : 0      counter subtraction
 *   PG_COMBINE_LEFT  b > 0 ? a : 0          intersection, a's counts
 *   PG_COMBINE_ONLY  b == 0 ? a : 0         k-mer subtraction
 *   PG_COMBINE_KEEP  a                      a filter; b must be NULL (and must not be for the others)
 * Sources are only read (plain loads); a and b may be the same table.  All three entries are additive to ABI 9; every argument
 * is checked before anything is enqueued (PG_EINVAL with a pg_last_error text: a null table or status, differing k, a kind that
 * does not admit k, an unknown op, KEEP with a b or another op without, lower < 1, 0 <= upper < lower, data not 16-byte aligned,
 * dst aliasing a source, the aligned entry on tables pg_table_merge_aligned_applies does not pair, cap < 0).
 *   pg_table_combine_aligned  stands beside the tables of feature.py:76-94 (replaces nothing of the reference): dst, a and b are
 *                             all PG_TABLE_MINI, or all PG_TABLE_HASH in LDS-sized buckets, of one k and geometry
 *                             (pg_table_merge_aligned_applies(dst, a) and (dst, b) are 1).  One workgroup per bucket combines
 *                             the two slices inside LDS and writes the slice of dst once, 16 bytes per store -- only streams, no
 *                             global atomics.  dst is REBUILT: its old content is neither read nor need be initialised, and a
 *                             bucket that loses entries has its probing chains built anew.  Only PG_COMBINE_MAX can run out of
 *                             room: a bucket whose union does not fit sets PG_STATUS_TABLE_FULL in status[0] (device
 *                             uint32_t[2], zeroed by the caller; dst is then incomplete: take pg_table_combine_items).
 *   pg_table_combine_items    stands beside the tables of feature.py:76-94 and the dump count_kmer.cpp:139-170 reads
 *                             (replaces nothing of the reference), general form: every entry of `a` is looked up in `b`, whatever
 *                             the two kinds and geometries, and the survivors leave as items codes[i] (canonical code), counts[i] = r,
 *                             in no particular order, at i = the old n_out[0] and up; n_out[0] (device, zeroed by the caller
 *                             before the first call) grows by the number of survivors.  An item at cap or beyond is not stored
 *                             and sets PG_STATUS_OVERFLOW_LIST in status[0]; cap = a's entries always suffices.  r is not
 *                             clamped: a value that enters a packed table is clamped to PG_HASH_COUNT_SAT by the insert
 *                             (pg_kmer_merge).  PG_COMBINE_MAX emits max(a, b) for the entries of `a` only: the union is that
 *                             call followed by (b, a, PG_COMBINE_ONLY) -- every k-mer leaves exactly one of the two.
 *   pg_table_compare          stands beside the tables of feature.py:76-94 (replaces nothing of the reference): one pass over
 *                             `a` that looks every entry up in `b` -- out[0] = a's entries, out[1] = the sum of a's counts, out[2] = entries b
 *                             holds too, out[3] = the sum of min(a, b) (device uint64_t[4], cleared on `stream` first and
 *                             written whole).  b == NULL: out[2] = out[3] = 0.
 * ---------------------------------------------------------------------------------------------- */
#define PG_COMBINE_MIN 0
#define PG_COMBINE_MAX 1
#define PG_COMBINE_DIFF 2
#define PG_COMBINE_LEFT 3
#define PG_COMBINE_ONLY 4
#define PG_COMBINE_KEEP 5
int pg_table_combine_aligned(const pg_table *dst, const pg_table *a, const pg_table *b /* NULL: keep */, int op,
                             int64_t lower, int64_t upper /* < 0: none */, uint32_t *status, void *stream);
int pg_table_combine_items(const pg_table *a, const pg_table *b /* NULL: keep */, int op, int64_t lower, int64_t upper,
                           uint64_t *codes, uint32_t *counts, int64_t cap, int64_t *n_out /* device [1] */,
                           uint32_t *status, void *stream);
int pg_table_compare(const pg_table *a, const pg_table *b /* may be NULL */, uint64_t *out /* device [4] */, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Per-run feature rows (device).  One launch fills both matrices.
 *   tnf_out [n_rows, ncols(k_tnf)] int32: canonical k_tnf-mer counts        (count_tnf.cpp:78-113)
 *   abd_out [n_rows, vsize]        int32: hist[count(kmer)/window]++ where the bin is < vsize
 *                                          (count_kmer.cpp:55-108)
 * Either output may be NULL (then its parameters are ignored).  Both must be zero-filled by the
 * caller; segments of one row add into the same row.  seg_* are the device copies of
 * pg_plan_segments' arrays; colmap is the device copy of pg_tnf_colmap's table.
 * ---------------------------------------------------------------------------------------------- */
int pg_features(const uint64_t *codes, const uint32_t *valid, int64_t n_words,
                const int32_t *seg_row, const int64_t *seg_start, const int64_t *seg_end, int64_t n_segs,
                int k_tnf, const uint16_t *colmap, int32_t *tnf_out,
                const pg_table *t, int window, int vsize, int32_t *abd_out, void *stream);

/* The abundance matrix of pg_features WITHOUT random table reads (count_kmer.cpp:55-108 again): the records left in
 * `count_workspace` by pg_kmer_count_bucketed(..., rows, ...) are looked up bucket by bucket in LDS copies of the
 * table's slices (so `t` may meanwhile have been merged with other ranks' tables), turned into (row, bin) words,
 * scattered back by groups of 64 rows and histogrammed in LDS.  abd_out [n_rows, vsize] is overwritten (no zero
 * fill needed).  Requirements: the same `t` geometry, `rows` and word count as the counting call, one counting
 * call since the table was last reset, vsize <= PG_SHUFFLE_MAX_VSIZE.  workspace: pg_abundance_workspace_bytes. */
#define PG_SHUFFLE_MAX_VSIZE 512
int64_t pg_abundance_workspace_bytes(int64_t n_words_counted, int64_t n_rows, int vsize, const pg_table *t);
int pg_abundance_from_records(const pg_table *t, const pg_rows *rows, int window, int vsize, int32_t *abd_out,
                              const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                              void *workspace, int64_t workspace_bytes, void *stream);
int pg_abundance_from_emitted(const pg_table *t, const pg_rows *rows, int window, int vsize, int32_t *abd_out,
                              const void *count_workspace, int64_t count_workspace_bytes, int64_t n_words_counted,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * The super-k-mer form of the table build + abundance lookups (one GPU, PG_TABLE_MINI; same results as
 * pg_kmer_count_bucketed_emit + pg_abundance_from_emitted, i.e. jellyfish count -C (feature.py:94) and
 * count_kmer.cpp:55-108).
 *   pg_mini_plan   one pass over the word range: how many super-k-mer records every CHUNK of the stream sends to each
 *                  first-pass region and how many records every bucket receives -> exact write offsets for both scatter
 *                  passes (no global cursor atomics in the first one).  Depends on the stream, `rows` and the table
 *                  geometry only: a caller that counts the same range again (another pass, a benchmark step) keeps the
 *                  plan.  Leaves the number of records in the first 8 bytes of `plan_ws` (device).
 *   pg_mini_count  stream -> records by region -> records by bucket -> every bucket counted inside LDS by one
 *                  workgroup (slots of a FRESH table are overwritten, no clearing) and, when window > 0, looked up again
 *                  while its counts are still in LDS: the (row, bin) words of count_kmer.cpp:86-96 are left in
 *                  `shuffle_ws` for pg_mini_abundance_from_emitted.  `rows` may be NULL and window = vsize = 0 (table only).
 * plan_ws: pg_mini_plan_bytes; rec_ws: pg_mini_records_bytes(n_records, t) (two buffers of 12 B per record);
 * shuffle_ws: pg_mini_shuffle_bytes.  All 256-byte aligned
 * device memory.  A plan that names more records than rec_ws holds sets PG_STATUS_PLAN_MISMATCH and counts nothing.
 * ---------------------------------------------------------------------------------------------- */
int64_t pg_mini_plan_bytes(int64_t n_words, const pg_table *t);
int pg_mini_plan(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                 const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *stream);
int64_t pg_mini_records_bytes(int64_t n_records, const pg_table *t);
int64_t pg_mini_shuffle_bytes(int64_t n_words, int64_t n_rows, int vsize);
/* the same for a caller that passes merge_ws to pg_mini_count: where the merged lookups apply (the library's own rule: the slot
 * form, fewer than 2^20 rows, row and bin in 28 bits) and the row groups take one scatter pass, the row shuffle's buffer of
 * provisional words is not part of the layout -- half the bytes (12 GB less per 10 M read pairs) */
int64_t pg_mini_shuffle_bytes_merged(int64_t n_words, int64_t n_rows, int vsize, const pg_table *t);
/* merge_ws (may be NULL: the word-wise lookups): pg_mini_merge_words() 4-byte words of device memory for the MERGED form of the
 * lookups (the default; PG_MINI_MERGE=0 in the environment or a NULL buffer: word-wise) -- the k-mers of a record that share row
 * and bin travel as one word with a count; the provisional data are the k-mers' 2-byte slot numbers in fixed places per record,
 * sized from the plan's record counts (the plan workspace's first 8-byte word: records; third: records of more than 4 k-mers). */
int64_t pg_mini_merge_words(int64_t n_words, int64_t n_records, int64_t n_long_records, const pg_table *t);

/* ---- a stream counted in PIECES (one GPU, packed mini tables, the merged lookups): the scratch of pg_mini_count grows with the
 * stream (about 3.4 KB per 150 bp read pair); a stream too large for one piece is counted word range by word range.  The reference
 * streams one barcode group at a time in O(group) memory (count_tnf.cpp:257-271) and needs the finished jellyfish table before the
 * first lookup (count_kmer.cpp:139-170); here every piece is planned, partitioned and counted INTO the table's buckets (the bucket's
 * slice is loaded into LDS, counted on, written back: slots keep their places), leaving only its 2-byte provisional slots and the
 * meta words of its records behind; when the table is final the pieces' slots are looked up in it:
 *   pg_mini_plan(codes, valid, w0, w1, ...)      the piece's plan (its own plan_ws, kept until the lookups)
 *   pg_mini_count_piece(... first ...)          plan_ws, rec_ws, merge_ws of THIS piece; first != 0 for the first piece of a fresh table
 *   (keep: plan_ws, merge_ws and the second meta plane of rec_ws -- records x 4 bytes -- of every piece)
 *   pg_mini_lookup_begin(t, rows, n_words_total, vsize, shuffle_ws, ...)   once; shuffle_ws: pg_mini_shuffle_bytes_merged(n_words_total, ...)
 *   pg_mini_lookup_piece(...)                   per piece, any order
 *   pg_mini_abundance_from_emitted(t, rows, vsize, abd, <a plan_ws of pg_mini_plan_bytes(n_words_total)>, ..., n_words_total, shuffle_ws, ...)
 * rows: the rows of the WHOLE stream (their positions are absolute). */
int pg_mini_count_piece(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                        const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                        int window, int vsize, void *merge_ws, int64_t merge_ws_words, int first, uint32_t *status, void *stream);
int pg_mini_lookup_begin(const pg_table *t, const pg_rows *rows, int64_t n_words_total, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *stream);
int pg_mini_lookup_piece(const pg_table *t, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_piece,
                         const uint32_t *meta, int64_t n_words_total, int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes,
                         const void *merge_ws, uint32_t *status, void *stream);
int pg_mini_count(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                  const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                  int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                  uint32_t *status, void *stream);
/* `stream` waits for the first scatter pass of the calling thread's latest pg_mini_count (an event recorded there): the next
 * batch's pg_mini_plan, enqueued on that stream afterwards, runs beside the memory-bound second pass. */
int pg_mini_wait_first_pass(void *stream);
int pg_mini_abundance_from_emitted(const pg_table *t, const pg_rows *rows, int vsize, int32_t *abd_out,
                                   const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_counted,
                                   void *shuffle_ws, int64_t shuffle_ws_bytes, void *stream);

/* ---- the super-k-mer form on N > 1 ranks (the reference runs ONE jellyfish over all reads: feature.py:94; here every rank
 * counts its own reads and the counts meet at bucket owners).  A rank's counts are not final until the other ranks' occurrences
 * of the same k-mers are in, so pg_mini_count is cut in two:
 *   pg_mini_count_half    as pg_mini_count up to the bucket workgroups, which leave -- instead of the slice and the lookups --
 *                         their occupied slots (canonical code << 22 | count) as compacted ENTRIES in slot order, the number of
 *                         them in fill[bucket] (device int64), the occupancy bitmaps and the provisional (row, slot) words.
 *                         `local` has the UNION's bucket count and, per bucket, slots for this rank's own k-mers; its `data` is
 *                         never written.
 *   pg_mini_gather_entries  bucket b's entries -> out[dst_elem[b] ..): the send buffer (out_elems entries), bucket ranges in owner order
 *   (all-to-all: 8 bytes per entry)
 *   pg_mini_merge_bins    owner side, buckets [bucket_begin, bucket_end) of the union table `t`: part p's entries of owned bucket i
 *                         lie at recv[p * part_stride + seg[p * (n_owned + 1) + i] .. seg[p * (n_owned + 1) + i + 1]); the parts are
 *                         summed inside LDS (counts saturate at PG_HASH_COUNT_SAT, as one rank's would), the merged slices are
 *                         written to `t`, and bins_out (same layout, uint16) receives for EVERY entry the bin of its k-mer in the
 *                         merged table: count / window + 1, or 0xffff beyond the vector (count_kmer.cpp:86-96)
 *   (all-to-all back: 2 bytes per entry)
 *   pg_mini_lookup_half   bins_in[bin_elem[b] ..) = the bins of bucket b's entries, in the order they were sent -> the lookups of
 *                         the provisional words and the row-group scatter, exactly as pg_mini_count ends;
 *                         pg_mini_abundance_from_emitted(local, ...) then writes the rows.
 * half_ws: pg_mini_half_bytes(local), 256-byte aligned device memory; merge_ws as for pg_mini_count (the same buffer in both calls);
 * rec_ws: the count half's record workspace, untouched in between (the merged lookups read the records' lengths and rows again). */
int64_t pg_mini_half_bytes(const pg_table *local);
int pg_mini_count_half(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *local,
                       const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                       int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                       void *half_ws, int64_t half_ws_bytes, int64_t *fill, uint32_t *status, void *stream);
int pg_mini_gather_entries(const pg_table *local, const void *half_ws, int64_t half_ws_bytes, const int64_t *fill,
                           const int64_t *dst_elem, uint64_t *out, int64_t out_elems, uint32_t *status, void *stream);
int pg_mini_merge_bins(const uint64_t *recv, int64_t part_stride, const int64_t *seg, int n_parts, const pg_table *t,
                       int64_t bucket_begin, int64_t bucket_end, int window, int vsize, uint16_t *bins_out, uint32_t *status, void *stream);
int pg_mini_lookup_half(const pg_table *local, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, const void *rec_ws, int64_t rec_ws_bytes,
                        int64_t n_words_counted,
                        int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, const void *merge_ws, int64_t merge_ws_words,
                        const void *half_ws, int64_t half_ws_bytes,
                        const uint16_t *bins_in, const int64_t *bin_elem, uint32_t *status, void *stream);

/* ---- the count half in PIECES (N > 1 ranks): a rank whose share would not fit one piece of scratch counts it word range by word
 * range, as one GPU does (pg_mini_count_piece above; the reference streams one barcode group at a time, count_tnf.cpp:257-271, and
 * looks up in the finished table only, count_kmer.cpp:139-170).  The pieces count INTO the buckets of `local`, which has real slots
 * here (2^log2_slots words of device memory; slots keep their places from piece to piece); the LAST piece ends as
 * pg_mini_count_half ends: entries, occupancy and fill in half_ws, so that the exchange (pg_mini_gather_entries, pg_mini_merge_bins)
 * is the same as for one piece.  The calls:
 *   pg_mini_plan(codes, valid, w0, w1, local, ...)         the piece's plan (its own plan_ws, kept until its lookups)
 *   pg_mini_count_half_piece(... first, last ...)           plan_ws, rec_ws, merge_ws of THIS piece; first != 0 for the first piece,
 *                                                          last != 0 for the last (both: a single piece); fill zeroed by the caller
 *   (keep: plan_ws, merge_ws and the second meta plane of rec_ws -- records x 4 bytes from pg_mini_records_meta_offset -- of every
 *   piece; half_ws and fill until the lookups; the local slots may go after the last piece)
 *   ... the exchange, as for one piece ...
 *   pg_mini_lookup_begin(local, rows, n_words_total, vsize, shuffle_ws, ...)   once; shuffle_ws: pg_mini_shuffle_bytes_merged(n_words_total, ...)
 *   pg_mini_lookup_half_piece(...)                         per piece, any order (a bucket without records of the piece: nothing)
 *   pg_mini_abundance_from_emitted(local, rows, vsize, abd, <a plan_ws of pg_mini_plan_bytes(n_words_total)>, ..., n_words_total, ...)
 * Counts clamp at PG_HASH_COUNT_SAT across pieces as across the adds of one.  Workspaces: half_ws = pg_mini_half_bytes(local); per
 * piece pg_mini_plan_bytes(piece words), pg_mini_records_bytes(records) (reused from piece to piece), pg_mini_merge_words(...).
 * A piece needs the merged lookups (pg_mini_merge_form_applies). */
int pg_mini_count_half_piece(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *local,
                             const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                             int window, int vsize, void *merge_ws, int64_t merge_ws_words, void *half_ws, int64_t half_ws_bytes,
                             int64_t *fill, int first, int last, uint32_t *status, void *stream);
int pg_mini_lookup_half_piece(const pg_table *local, const pg_rows *rows, const void *plan_ws, int64_t plan_ws_bytes, int64_t n_words_piece,
                              const uint32_t *meta, int64_t n_words_total, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes,
                              const void *merge_ws, const void *half_ws, int64_t half_ws_bytes,
                              const uint16_t *bins_in, const int64_t *bin_elem, uint32_t *status, void *stream);
/* 1 where the merged lookups apply to n_rows rows with this vector size on the table's geometry (the slot form: fewer than
 * 2^(32 - log2_bucket_slots) - 1 rows; fewer than 2^20 rows; row bits + bin bits + 6 <= 28, i.e. at most 2^19 rows at vsize 400;
 * PG_MINI_MERGE=0 in the environment: never), 0 where they do not, < 0 for a bad table: the rule every pieces entry checks */
int pg_mini_merge_form_applies(const pg_table *t, int64_t n_rows, int vsize);
/* ---- abundance rows against a FINISHED table, in super-k-mer form.  Replaces count_kmer -g DUMP: the per-occurrence lookups of
 * cpptools/count_kmer.cpp:55-108 in a table that was loaded, merged or counted from other reads (count_kmer.cpp:139-170); a k-mer
 * the table does not hold adds nothing (count_kmer.cpp:87).  pg_mini_count answers a bucket's lookups while it counts the bucket,
 * which only serves the stream the table is counted from; here the bucket workgroup FINDS instead of inserting: the bucket's slice
 * of `t` is loaded into LDS, every k-mer of the stream's row-tagged records walks its probe chain read-only (home slot, linear,
 * wrapping inside the bucket, until its key or an empty slot), and the slots found are looked up as the fused kernel looks up the
 * slots it made.  `t` is never written.
 *   pg_mini_find_applies  the one statement of where the form applies: 1 for a PG_TABLE_MINI table (PG_MINI_MIN_K <= k <= 21) where
 *                         pg_mini_merge_form_applies(t, n_rows, vsize) is 1, 1 <= window, 1 <= vsize <= PG_SHUFFLE_MAX_VSIZE and
 *                         window * vsize <= PG_HASH_COUNT_SAT; 0 otherwise; < 0 for a bad descriptor.
 *   pg_mini_find          the calls and workspaces of pg_mini_count -- the same pg_mini_plan (of the stream whose rows are wanted, on
 *                         the table's geometry), plan_ws, rec_ws, shuffle_ws (pg_mini_shuffle_bytes_merged) and merge_ws
 *                         (pg_mini_merge_words) --, `rows` required.  Leaves the (row, bin) words in shuffle_ws for
 *                         pg_mini_abundance_from_emitted.  PG_EINVAL, before anything is enqueued, for null rows, a table of
 *                         another kind, workspaces too small or not 256-byte aligned, and where pg_mini_find_applies is not 1.
 *                         status[0]: PG_STATUS_PLAN_MISMATCH as for pg_mini_count; PG_STATUS_TABLE_FULL when a k-mer that the table
 *                         lacks met a bucket of 2^13 (2^14: the 1024-thread form) slots without one free slot -- the words are
 *                         then incomplete and the rows must come from pg_features. */
int pg_mini_find_applies(const pg_table *t, int64_t n_rows, int window, int vsize);
int pg_mini_find(const uint64_t *codes, const uint32_t *valid, int64_t word_begin, int64_t word_end, const pg_table *t,
                 const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                 int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                 uint32_t *status, void *stream);
/* byte offset of the second meta plane ("meta B": the bucket-ordered records' meta words that the pieces keep) inside a record
 * workspace of rec_ws_bytes bytes: [bases A | bases B | meta A | meta B] of the largest capacity that fits, a multiple of 256 */
int64_t pg_mini_records_meta_offset(int64_t rec_ws_bytes, const pg_table *t);

/* ---- the super-k-mer form on N > 1 ranks for MASKED input: soft-masked reads counted with lower-case bases (jellyfish count -C,
 * feature.py:94) and paired reads whose bases below the quality threshold jellyfish reads as N (--min-qual-char=?, feature.py:76-83),
 * while the reference's own row counters take neither rule (count_kmer.cpp:55-108).  Two planes then decide about a k-mer:
 *   T  its bases are valid under `table_valid`: it counts +1 in the multiplicity table;
 *   R  its bases are valid under rows->strict_valid (NULL: `valid`): it belongs to the row it lies in and its bin is looked up.
 * `valid` is the plane U = table_valid | strict plane.  A k-mer is kept if T holds, or R inside a row; records are also cut where T
 * changes.  A record of R-and-not-T k-mers takes local slots as any record but adds 0 to their counts, so the count half's entries
 * may carry count 0; the owner merge of this form inserts every entry with count > 0, then LOOKS UP the count-0 ones: a key that no
 * rank counted has no bin (count_kmer.cpp:87 skips a k-mer missing from the dump).  The merged slices hold counted k-mers only.
 * The calls and workspaces are those of the plain form (pg_mini_plan / pg_mini_count_half / pg_mini_merge_bins, pieces included)
 * with the _masked entries below in their places; table_valid = NULL is the plain form.  The masked count half needs the merged
 * lookups (pg_mini_merge_form_applies) and at most PG_MINI_MASKED_MAX_ROWS rows, else PG_EINVAL.  It clears the row-only flag in the
 * meta plane it leaves (meta B), which the lookup half and the kept meta words of pieces read as usual.  The owner merge must be the
 * masked one on EVERY rank as soon as any rank's count half is: pg_mini_merge_bins_masked also takes plain parts. */
int pg_mini_plan_masked(const uint64_t *codes, const uint32_t *valid, const uint32_t *table_valid, int64_t word_begin, int64_t word_end,
                        const pg_table *t, const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *stream);
int pg_mini_count_half_masked(const uint64_t *codes, const uint32_t *valid, const uint32_t *table_valid, int64_t word_begin, int64_t word_end,
                              const pg_table *local, const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                              int window, int vsize, void *shuffle_ws, int64_t shuffle_ws_bytes, void *merge_ws, int64_t merge_ws_words,
                              void *half_ws, int64_t half_ws_bytes, int64_t *fill, uint32_t *status, void *stream);
int pg_mini_count_half_piece_masked(const uint64_t *codes, const uint32_t *valid, const uint32_t *table_valid, int64_t word_begin, int64_t word_end,
                                    const pg_table *local, const pg_rows *rows, void *plan_ws, int64_t plan_ws_bytes, void *rec_ws, int64_t rec_ws_bytes,
                                    int window, int vsize, void *merge_ws, int64_t merge_ws_words, void *half_ws, int64_t half_ws_bytes,
                                    int64_t *fill, int first, int last, uint32_t *status, void *stream);
int pg_mini_merge_bins_masked(const uint64_t *recv, int64_t part_stride, const int64_t *seg, int n_parts, const pg_table *t,
                              int64_t bucket_begin, int64_t bucket_end, int window, int vsize, uint16_t *bins_out, uint32_t *status, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Row normalisation of a count matrix (a9: Data.__init__, src/data.py:16-21 -- sklearn normalize(norm="l1") in float64, the
 * sampling weight = (row maximum of the normalised abundance)^2, matrices narrowed to float32).  One pass over device int32
 * [n_rows, n_cols]: out[r, c] = (float)((double)m[r, c] / (double)sum_c |m[r, c]|), an all-zero row stays zero (sklearn puts 1
 * for a zero norm); weight[r] (may be NULL) = ((double)max_c m[r, c] / sum)^2 -- division by a positive number is monotone, so
 * this is the square of the row maximum of the quotients.  Integer sums and IEEE double division: bit-identical to the CPU.
 * ---------------------------------------------------------------------------------------------- */
int pg_normalize_rows(const int32_t *m, int64_t n_rows, int n_cols, float *out, double *weight, void *stream);

/* ----------------------------------------------------------------------------------------------
 * An affine map of the rows of two matrices that lie side by side (additive to ABI 9): the eval-mode VAE encoder, whose
 * Linear / BatchNorm1d (running statistics) / LeakyReLU(slope 1) / Dropout layers and l_mu fold into one matrix and one
 * offset (pangaea_amd/models/VAENET.py: affine_encoder).  Device float32 abd [n_rows, n_abd] and tnf [n_rows, n_tnf], both
 * contiguous; device float64 w [(n_abd + n_tnf), n_out] and b [n_out]; device float32 out [n_rows, n_out]:
 *     out[r, :] = (float)([abd[r, :], tnf[r, :]] . w + b)
 * Products and sums in float64, each output one chain of fused multiply-adds over the inputs in order, starting from b, and
 * narrowed once: the bits of a row do not depend on n_rows or on where in the batch it lies.  Checked before anything is
 * enqueued (PG_EINVAL, the argument named in pg_last_error): n_abd, n_tnf >= 0 with n_abd + n_tnf >= 1,
 * 1 <= n_out <= PG_AFFINE_MAX_OUT, n_rows >= 0, no null pointer (abd / tnf may be null when it has no columns).
 * n_rows == 0: PG_OK, nothing enqueued.
 * ---------------------------------------------------------------------------------------------- */
#define PG_AFFINE_MAX_OUT 64
int pg_affine_rows(const float *abd, int n_abd, const float *tnf, int n_tnf, int64_t n_rows, const double *w, const double *b, int n_out,
                   float *out, void *stream);
/* One step of the fold that produces w and b, from the back (additive to ABI 9).  In front of the map out = y . a + c stands
 * the eval-mode layer y = BatchNorm1d(Linear(h)): device float32 weight [n_mid, n_in], bias [n_mid] (NULL: none), the
 * BatchNorm1d's running mean and variance [n_mid] (both NULL: no BatchNorm1d), gamma and beta [n_mid] (NULL: 1 and 0) and its
 * eps; device float64 a [n_mid, n_out] (NULL: the identity, n_mid == n_out) and c [n_out] (NULL: zeros).  With
 * s = gamma / sqrt(var + eps):
 *     a_out[i, o] = sum_j weight[j, i] * s[j] * a[j, o]        c_out[o] = c[o] + sum_j ((bias[j] - mean[j]) * s[j] + beta[j]) * a[j, o]
 * device float64 a_out [n_in, n_out] and c_out [n_out] (neither may overlap a or c), all contiguous, in float64, one launch.
 * PG_EINVAL with the argument named: sizes outside [1, 2^24], n_out > PG_AFFINE_MAX_OUT, a null weight, a_out or c_out, a mean
 * without a variance, gamma or beta without a mean, a null a with n_mid != n_out. */
int pg_affine_fold(const float *weight, const float *bias, const float *bn_mean, const float *bn_var, const float *bn_gamma,
                   const float *bn_beta, double bn_eps, int n_in, int n_mid, const double *a, const double *c, int n_out,
                   double *a_out, double *c_out, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Pairwise-distance sums per cluster (additive to ABI 9): the O(N^2) part of the silhouette score by which
 * pangaea_amd/clustering.py: choose_clusters picks the number of clusters (the sweep whose parameters the reference's
 * cluster_barcode_reads still carries -- range_step, patience, delta, src/clustering.py:70 -- next to its unused import of
 * silhouette_score, src/clustering.py:5).  Device float32 q [n_q, dim] and x [n_x, dim], contiguous, x SORTED by cluster;
 * device int64 seg [k + 1] with seg[0] == 0, seg[k] == n_x, non-decreasing (rows seg[c] .. seg[c+1]-1 of x are cluster c; empty
 * clusters anywhere); device float64 out [n_q, k]:
 *     out[i][c] = sum over j in cluster c of |q_i - x_j|_2
 * |q_i - x_j| from the differences (subtract, square, accumulate over dim in float32, one square root), never from
 * |q|^2 + |x|^2 - 2 q.x; the sum over j in float64, float32 partial sums of at most PG_CLUSTER_GROUP distances folded into it.
 * A sum over an empty cluster and a sum over rows identical to q_i are exactly 0.  The reference range is cut into n_splits
 * pieces [n_x * s / n_splits, n_x * (s + 1) / n_splits), one set of workgroups each (0: the library chooses, one when the query
 * rows alone fill the device; > 0: forced); with more than one, every piece writes its own [n_q, k] plane into the workspace
 * and the planes are added in order of s: no floating-point atomics, the same bits from run to run for the same arguments.
 * pg_cluster_dist_sums_workspace_bytes: what that takes (0 with one split; at most n_splits * n_q * k * 8), or PG_EINVAL.
 * dim == 32 (the -ld default) keeps the query row in registers; every other dim takes a generic loop.
 * Checked before anything is enqueued (PG_EINVAL, the argument named in pg_last_error): n_q, n_x >= 0, 1 <= dim <=
 * PG_CLUSTER_MAX_DIM, 1 <= k <= PG_CLUSTER_MAX_K, 0 <= n_splits <= PG_CLUSTER_MAX_SPLITS, no null q, x, seg or out, a workspace of
 * the size above.  seg lies on the device and is not looked at by the host (its caller built it); the kernel clamps its values
 * into the range of its piece, so whatever it holds, nothing outside x is read.  n_q == 0 or n_x == 0: PG_OK, nothing enqueued,
 * out untouched.
 * ---------------------------------------------------------------------------------------------- */
#define PG_CLUSTER_MAX_DIM 256
#define PG_CLUSTER_MAX_K 4096
#define PG_CLUSTER_MAX_SPLITS 64
#define PG_CLUSTER_GROUP 8
int64_t pg_cluster_dist_sums_workspace_bytes(int64_t n_q, int64_t n_x, int k, int n_splits);
int pg_cluster_dist_sums(const float *q, int64_t n_q, const float *x, int64_t n_x, int dim, const int64_t *seg, int k, int n_splits,
                         double *out, void *workspace, int64_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Cache files.  Rows as the reference binaries print them: "<name>,v1,...,vD\n", numbers through
 * ostream<<double (%g, six significant digits; count_tnf.cpp:293-303), gzip container.
 * names: n_rows NUL-terminated strings back to back.  mat: host int32 [n_rows, n_cols].
 * ---------------------------------------------------------------------------------------------- */
int pg_write_csv_gz(const char *path, const char *names, const int32_t *mat, int64_t n_rows, int64_t n_cols);

/* ----------------------------------------------------------------------------------------------
 * Bin writer (host): clusters.tsv -> <out_prefix>_bin<label>.fq and .barcode, the on-disk bin layout the
 * unchanged reassembly stage reads.  Replaces the reference's extract_reads tool (extract_reads.cpp:57-190):
 * same tsv grammar ("-1" labels skipped), same kept pairs, same rewritten headers
 * ("<name>\tBX:Z:<barcode>-1").  r2 == NULL: interleaved input.  pairs_written may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int pg_extract_reads(const char *r1_or_interleaved, const char *r2_or_null, const char *clusters_tsv,
                     const char *out_prefix, int64_t *pairs_written);

#ifdef __cplusplus
}
#endif
#endif /* PANGAEA_FEAT_H */
