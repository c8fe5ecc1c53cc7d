"""The read verbs of a finished k-mer table (kmc_tools filter, khmer's filter-abund / trim-low-abund / normalize-by-median, BBNorm,
single-base correction): per-record rows of a FASTQ text on the device (``read_hits``, ``read_spans``, ``read_corrections``,
``read_depths``) and whole files through the device in pieces (``filter_fastq``, ``trim_fastq``, ``correct_fastq``,
``normalize_fastq``).  ``KmerTable`` takes these eight as its methods by assignment, so their first parameter is the table and is
called ``self``; the helpers beside them call it ``table``.  The FASTQ plumbing -- pieces, line index, rounds, the piece loop -- is
``fastqtext``; this module adds what a verb does with a round: a *step* (its kernel, its verdict, its bytes) and ``_TableRounds``."""
from __future__ import annotations

import os
import time

import numpy as np
import torch

from . import _lib, fastqtext
from .fastqtext import fastq_error, stream_ptr

# places in the totals of the piece loop: ONE int64 tensor on the device, added to by every step and read once at the end
(RECORDS, KEPT, PASSED, BASES, KMERS, HITS, TRIMMED, BASES_OUT, CANDIDATES, CORRECTED, READS_CORRECTED, LOW, DEPTH_IN,
 DEPTH_OUT) = range(14)
N_TOTALS = 14


def _hits_window(lower, upper, min_qual_char) -> tuple:
    """(lower, upper or -1, quality threshold byte or 0) as pg_table_read_hits takes them"""
    lower = int(lower)
    if lower < 0:
        raise ValueError(f"lower must be at least 0 (got {lower})")
    if upper is not None and int(upper) < lower:
        raise ValueError(f"upper ({upper}) is below lower ({lower})")
    if min_qual_char is None:
        mq = 0
    else:
        c = min_qual_char.encode("latin-1") if isinstance(min_qual_char, str) else bytes([min_qual_char]) if isinstance(min_qual_char, int) else bytes(min_qual_char)
        if len(c) != 1 or c[0] == 0:
            raise ValueError(f"min_qual_char must be one character (got {min_qual_char!r})")
        mq = c[0]
    return lower, -1 if upper is None else int(upper), mq


def _span_mode(mode) -> int:
    if mode not in _lib.SPAN_MODES:
        raise ValueError(f"mode must be first or longest (got {mode!r})")
    return _lib.SPAN_MODES[mode]


def _depth_args(lower, percentile, min_qual_char) -> tuple:
    """(lower, percentile, quality threshold byte or 0) as pg_table_read_depths takes them"""
    for name, v in (("lower", lower), ("percentile", percentile)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an int (got {v!r})")
    if lower < 1:
        raise ValueError(f"lower must be at least 1 (got {lower})")
    if not 0 <= percentile <= 100:
        raise ValueError(f"percentile must lie in [0, 100] (got {percentile})")
    return int(lower), int(percentile), _hits_window(1, None, min_qual_char)[2]


def _hit_bound(v, name: str) -> tuple:
    """a hit bound of ``KmerTable.filter_fastq`` as (is a share, value): an int is absolute, a float in [0, 1] a share of n"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be an int (absolute) or a float in [0, 1] (a share of the read's k-mers), got {v!r}")
    if isinstance(v, (int, np.integer)):
        if v < 0:
            raise ValueError(f"{name} must be at least 0 (got {v})")
        return False, int(v)
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"{name} as a share must lie in [0, 1] (got {v})")
    return True, float(v)


def _bound_holds(h: torch.Tensor, n: torch.Tensor, bound: tuple, at_least: bool) -> torch.Tensor:
    """h >= bound (``at_least``) or h <= bound, element-wise; a share is compared as h against f * n in IEEE double (h, n < 2^32:
    both sides exact before the product is rounded once, as numpy rounds it)"""
    share, v = bound
    ref = n.to(torch.float64) * v if share else v
    left = h.to(torch.float64) if share else h
    return left >= ref if at_least else left <= ref


def _fastq_files(src1, out1, src2, out2, pair: str) -> tuple:
    """(input paths, output paths) of ``KmerTable.filter_fastq`` / ``trim_fastq``, refused before anything is opened where they make
    no sense"""
    if pair not in ("any", "both", "single"):
        raise ValueError(f"pair must be any, both or single (got {pair!r})")
    if (src2 is None) != (out2 is None):
        raise ValueError("src2 and out2 go together: two inputs give two outputs")
    if pair == "single" and src2 is not None:
        raise ValueError("pair='single' judges the records of ONE file; R1/R2 input is paired")
    srcs = [os.fspath(src1)] + ([os.fspath(src2)] if src2 is not None else [])
    outs = [os.fspath(out1)] + ([os.fspath(out2)] if out2 is not None else [])
    fastqtext.check_outputs(outs, srcs, "the kept reads")
    return srcs, outs


# ---------------------------------------------------------------------------------------- a verb's step

class _Step:
    """what a verb does with the records of a text: ``rows`` enqueues its per-record entry, ``judge`` turns the entry's rows into pass
    flags and totals, ``sizes`` gives the bytes each kept record leaves with and ``gather`` writes them to their places.  Here:
    the launcher of all four entries, and records that leave whole (pg_fastq_gather).  ``window``: the entry's two numbers and
    the quality threshold byte"""

    def __init__(self, table, window, lenient):
        self.table, self.window, self.lenient = table, window, lenient

    def _launch(self, entry: str, text, n_bytes, idx, n_records, first_record, tail: tuple, status=None, events=None) -> torch.Tensor:
        """enqueue ``entry`` -- the table, the text with its line index, the records, the window, ``tail`` (the entry's own arguments
        and outputs), the status -- and return the status: int64 [2] on the device.  ``status``: a tensor to use (the entry
        writes it whole); ``events``: two device events recorded right around the entry"""
        table = self.table
        if status is None:
            status = torch.empty(2, dtype=torch.int64, device=table.device)
        a, b, mq = self.window
        call = getattr(_lib.load(), entry)
        if events:
            events[0].record()
        rc = call(table.desc(), table.k, text.data_ptr(), n_bytes, idx.data_ptr(), n_records, first_record, a, b, 1 if self.lenient else 0, mq,
                  *tail, status.data_ptr(), stream_ptr(table.device))
        if events:
            events[1].record()
        _lib.check(rc)
        return status

    def launch(self, s, n, status, events):
        """the entry on the first ``n`` records of a piece"""
        return self.rows(s.text, s.have, s.idx, n, s.done, status, events)[0]

    def sizes(self, s, rows, kept, tot):
        return s.idx[4 * kept + 4] - s.idx[4 * kept]

    def gather(self, s, n, rows, kept, dst, n_kept, out):
        return _lib.load().pg_fastq_gather(s.text.data_ptr(), s.have, s.idx.data_ptr(), n, kept.data_ptr(), dst.data_ptr(), n_kept, out.data_ptr(),
                                           out.numel(), stream_ptr(self.table.device))


class _HitsStep(_Step):
    """what ``KmerTable.filter_fastq`` does with a piece (``_TableRounds``): pg_table_read_hits, the hit bounds, the records byte
    for byte"""

    def __init__(self, table, window, lenient, lo_bound=None, hi_bound=None):
        super().__init__(table, window, lenient)
        self.lo_bound, self.hi_bound = lo_bound, hi_bound

    def rows(self, text, n_bytes, idx, n_records, first_record, status=None, events=None) -> tuple:
        """(hits: int32 [n_records, 2] holding the 32-bit counts, status) of pg_table_read_hits, both on the device"""
        hits = torch.empty((n_records, 2), dtype=torch.int32, device=self.table.device)
        return hits, self._launch("pg_table_read_hits", text, n_bytes, idx, n_records, first_record, (hits.data_ptr(),), status, events)

    def judge(self, hits, tot):
        nk, hh = (hits[:, 0].to(torch.int64) & 0xFFFFFFFF), (hits[:, 1].to(torch.int64) & 0xFFFFFFFF)
        ok = (nk >= 1) & _bound_holds(hh, nk, self.lo_bound, True)
        if self.hi_bound is not None:
            ok &= _bound_holds(hh, nk, self.hi_bound, False)
        tot[PASSED] += ok.sum()
        tot[KMERS] += nk.sum()
        tot[HITS] += hh.sum()
        return ok


class _SpansStep(_Step):
    """what ``KmerTable.trim_fastq`` does with a piece: pg_table_read_spans, span length >= min_len, the records cut to their spans
    (pg_fastq_gather_trimmed)"""

    def __init__(self, table, window, lenient, mode, min_len=None):
        super().__init__(table, window, lenient)
        self.mode, self.min_len = mode, min_len

    def rows(self, text, n_bytes, idx, n_records, first_record, status=None, events=None) -> tuple:
        """((spans: int32 [n_records, 4] holding the 32-bit n, h, start, length; trimmed bytes: int64 [n_records]), status) of
        pg_table_read_spans, all on the device"""
        spans = torch.empty((n_records, 4), dtype=torch.int32, device=self.table.device)
        sizes = torch.empty(n_records, dtype=torch.int64, device=self.table.device)
        return (spans, sizes), self._launch("pg_table_read_spans", text, n_bytes, idx, n_records, first_record,
                                            (self.mode, spans.data_ptr(), sizes.data_ptr()), status, events)

    def judge(self, rows, tot):
        wide = rows[0].to(torch.int64) & 0xFFFFFFFF
        ok = wide[:, 3] >= self.min_len
        tot[PASSED] += ok.sum()
        tot[KMERS] += wide[:, 0].sum()
        tot[HITS] += wide[:, 1].sum()
        return ok

    def sizes(self, s, rows, kept, tot):
        lens = rows[1][kept]
        tot[TRIMMED] += (lens < s.idx[4 * kept + 4] - s.idx[4 * kept]).sum()
        tot[BASES_OUT] += (rows[0][kept, 3].to(torch.int64) & 0xFFFFFFFF).sum()
        return lens

    def gather(self, s, n, rows, kept, dst, n_kept, out):
        return _lib.load().pg_fastq_gather_trimmed(s.text.data_ptr(), s.have, s.idx.data_ptr(), n, kept.data_ptr(), rows[0].data_ptr(), dst.data_ptr(),
                                                   n_kept, out.data_ptr(), out.numel(), stream_ptr(self.table.device))


class _CorrectStep(_Step):
    """what ``KmerTable.correct_fastq`` does with a piece: pg_table_correct_reads on the piece IN PLACE (the piece is the device's
    copy; what the host keeps for the next round is untouched), every record passes, and the records leave whole"""

    def rows(self, text, n_bytes, idx, n_records, first_record, out, status=None, events=None) -> tuple:
        """(rows: int32 [n_records, 4] holding the 32-bit n, h, candidates, corrected; status) of pg_table_correct_reads, both on the
        device.  ``out``: None (rows only), a copy of ``text`` or ``text`` itself (in place)"""
        rows = torch.empty((n_records, 4), dtype=torch.int32, device=self.table.device)
        return rows, self._launch("pg_table_correct_reads", text, n_bytes, idx, n_records, first_record,
                                  (None if out is None else out.data_ptr(), rows.data_ptr()), status, events)

    def launch(self, s, n, status, events):
        return self.rows(s.text, s.have, s.idx, n, s.done, s.text, status, events)[0]

    def judge(self, rows, tot):
        wide = rows.to(torch.int64) & 0xFFFFFFFF
        tot[PASSED] += wide.shape[0]
        tot[KMERS] += wide[:, 0].sum()
        tot[HITS] += wide[:, 1].sum()
        tot[CANDIDATES] += wide[:, 2].sum()
        tot[CORRECTED] += wide[:, 3].sum()
        tot[READS_CORRECTED] += (wide[:, 3] > 0).sum()
        return torch.ones(wide.shape[0], dtype=torch.bool, device=rows.device)


class _DepthsStep(_Step):
    """what ``KmerTable.normalize_fastq`` does with a piece: pg_table_read_depths (n, present, d and the unit's draw w per record),
    n >= 1 and d >= min_depth and w * d < target * 2^24 in exact 64-bit integers, the records byte for byte.  ``window``: what
    ``_depth_args`` gave"""

    def __init__(self, table, window, lenient, target=None, min_depth=None, seed=0, unit_log2=0):
        super().__init__(table, window, lenient)
        self.target, self.min_depth, self.seed, self.unit_log2 = target, min_depth, seed, unit_log2

    def rows(self, text, n_bytes, idx, n_records, first_record, status=None, events=None) -> tuple:
        """(rows: int32 [n_records, 4] holding the 32-bit n, present, d, w; status) of pg_table_read_depths, both on the device"""
        rows = torch.empty((n_records, 4), dtype=torch.int32, device=self.table.device)
        return rows, self._launch("pg_table_read_depths", text, n_bytes, idx, n_records, first_record,
                                  (self.seed, self.unit_log2, rows.data_ptr()), status, events)

    def judge(self, rows, tot):
        wide = rows.to(torch.int64) & 0xFFFFFFFF
        nk, d, w = wide[:, 0], wide[:, 2], wide[:, 3]
        low = (nk < 1) | (d < self.min_depth)
        ok = ~low & (w * d < self.target << 24)              # (w < 2^24, d < 2^32, target < 2^31: both sides below 2^56)
        tot[PASSED] += ok.sum()
        tot[KMERS] += nk.sum()
        tot[HITS] += wide[:, 1].sum()
        tot[LOW] += low.sum()
        tot[DEPTH_IN] += d.sum()
        return ok

    def sizes(self, s, rows, kept, tot):
        tot[DEPTH_OUT] += (rows[kept, 2].to(torch.int64) & 0xFFFFFFFF).sum()
        return super().sizes(s, rows, kept, tot)


# ---------------------------------------------------------------------------------------- a text on the device

def _rows_of_text(table, text: torch.Tensor, width: int, checked, rows_of) -> torch.Tensor:
    """what ``read_hits`` and its kin do with a text on the device: its checks, its line index, the rows
    ``rows_of(text, n_bytes, idx, n_records, checked())`` -> (int32 [n_records, width], status) widened to int64, and the
    ValueError for malformed text"""
    if not isinstance(text, torch.Tensor) or text.dtype != torch.uint8 or text.dim() != 1:
        raise TypeError("text must be a one-dimensional uint8 tensor")
    if not text.is_cuda:
        raise RuntimeError(f"the FASTQ text must live on a GPU: the k-mer kernels have no CPU path (got a tensor on {text.device})")
    table._require_readable()
    if text.device != table.device:
        raise ValueError("text and table are on different devices")
    args = checked()
    n = int(text.numel())
    if n == 0:
        return torch.zeros((0, width), dtype=torch.int64, device=table.device)
    text = text.contiguous()
    if text.data_ptr() & 15:                 # (a view into a larger text: the kernels read 16-byte pieces)
        text = text.clone()
    with torch.cuda.device(table.device):
        idx, n_lines = fastqtext.line_index(text, n)
        rows, bad = torch.zeros((0, width), dtype=torch.int32, device=table.device), -1
        if n_lines >= 4:
            rows, status = rows_of(text, n, idx, n_lines // 4, args)
            bad = int(status[1].item())
    if bad != -1:
        raise ValueError(fastq_error("the text", bad & ((1 << 64) - 1)))
    if n_lines % 4:
        raise ValueError(f"the text: record {n_lines // 4}: the text ends inside it ({n_lines} lines, no multiple of 4) (PG_EFORMAT)")
    return rows.to(torch.int64) & 0xFFFFFFFF


def read_hits(self, text: torch.Tensor, lower: int = 1, upper: int | None = None, lowercase_is_base: bool = True,
              min_qual_char=None) -> torch.Tensor:
    """(n, h) of every record of a four-line FASTQ text: int64 [n_records, 2] on the table's device -- n = the k-mers of the
    record's sequence line, h = those whose count c in this table (0: absent; saturated counts as stored) satisfies
    ``lower <= c <= upper`` (``upper`` None: no upper bound; ``lower`` 0 is allowed, ``lower = upper = 0`` counts the absent
    k-mers).  The alignment-free counterpart of the read choice of scripts/low_abd_reads.sh:10 (extract_unmapped.cpp).

    ``text``: a uint8 tensor ON THE DEVICE that holds whole records.  A line ends at ``\\n``, a last line without one is a
    line, ``\\r`` is an ordinary byte of its line (no base).  Record r is lines 4r .. 4r + 3; line 0 must begin with ``@``,
    line 2 with ``+``.  Position i of the sequence line holds a k-mer iff i + k <= its length and bytes i .. i + k - 1 are all
    bases: ACGT, and acgt too when ``lowercase_is_base`` (the rule the tables are counted with); with ``min_qual_char`` a
    base whose quality byte at the same offset is below it is no base (what ``--min-qual-char`` does to -1/-2 tables), and
    a quality line shorter than its sequence line is malformed -- otherwise the quality line is never looked at.  Malformed
    text (a line count that is no multiple of 4 included) raises ValueError naming the first offending record; a CPU tensor
    RuntimeError.  The table is only read (pg_fastq_index, pg_table_read_hits)."""
    return _rows_of_text(self, text, 2, lambda: _hits_window(lower, upper, min_qual_char),
                         lambda t, n, idx, n_rec, window: _HitsStep(self, window, bool(lowercase_is_base)).rows(t, n, idx, n_rec, 0))


def read_spans(self, text: torch.Tensor, lower: int = 1, upper: int | None = None, mode: str = "longest", lowercase_is_base: bool = True,
               min_qual_char=None) -> torch.Tensor:
    """(n, h, start, length) of every record of a four-line FASTQ text: int64 [n_records, 4] on the table's device -- n, h as
    ``read_hits`` gives them, and the record's solid span: position i of the sequence line is SOLID iff it holds a k-mer whose
    count c in this table satisfies ``lower <= c <= upper``; a run is a maximal interval [a, b) of solid positions and covers
    the bases [a, b + k - 1).  ``mode`` "longest": the longest run's (start, length) = (a, b - a + k - 1), among equals the
    leftmost; "first": the run that begins at position 0, i.e. the read up to its first k-mer outside the window
    (`kmc_tools filter -t`, khmer's filter-abund).  (0, 0) where there is no such run.  ``text``, the k-mer rules and the
    errors are those of ``read_hits``; in addition a quality line that does not reach as far as its sequence line (line
    ends aside) is malformed whatever ``min_qual_char`` says, since a trimmed record cuts it too.  The table is only read
    (pg_fastq_index, pg_table_read_spans)."""
    def rows_of(t, n, idx, n_rec, a):
        (spans, _), status = _SpansStep(self, a[0], bool(lowercase_is_base), a[1]).rows(t, n, idx, n_rec, 0)
        return spans, status

    return _rows_of_text(self, text, 4, lambda: (_hits_window(lower, upper, min_qual_char), _span_mode(mode)), rows_of)


def read_corrections(self, text: torch.Tensor, lower: int = 1, upper: int | None = None, lowercase_is_base: bool = True,
                     min_qual_char=None) -> tuple:
    """single-base substitutions of a four-line FASTQ text put right from this table (what khmer, Lighter, BFC and Musket do):
    (rows: int64 [n_records, 4] -- n, h, candidates, corrected --, the corrected text: uint8, a new tensor of the text's size;
    the argument is not modified), both on the table's device.  n and h are those of ``read_hits`` on the text as it came.

    A position of a sequence line (its bytes without a final ``\\r``) is SOLID iff it holds a k-mer whose count c in this
    table satisfies ``lower <= c <= upper``, WEAK iff it holds a k-mer whose count does not, VOID iff it holds none.  A
    CANDIDATE is a maximal run [a, b) of weak positions between two solid ones with b - a == k, or between a solid one and
    an end of the line with b - a <= k: the signature of ONE wrong base p (b - 1, or a + k - 1 at the right end) whose
    k-mers are all weak.  It is CORRECTED iff exactly one other base at p makes all b - a k-mers solid; that base goes into
    byte p in the letter case it had.  Runs beside a void position, runs of any other length (two errors closer than k) and
    reads that are weak throughout are left alone, as are candidates with no or several fitting bases; the quality line
    never changes.  All candidates of a record are judged on the record as it came: a second call corrects nothing more.
    ``text``, the k-mer rules and the errors are those of ``read_spans``.  The table is only read (pg_fastq_index,
    pg_table_correct_reads)."""
    fixed = []

    def rows_of(t, n, idx, n_rec, window):
        fixed.append(t.clone())
        return _CorrectStep(self, window, bool(lowercase_is_base)).rows(t, n, idx, n_rec, 0, fixed[0])

    rows = _rows_of_text(self, text, 4, lambda: _hits_window(lower, upper, min_qual_char), rows_of)
    return rows, fixed[0] if fixed else text.clone()


def read_depths(self, text: torch.Tensor, lower: int = 1, percentile: int = 50, lowercase_is_base: bool = True,
                min_qual_char=None) -> torch.Tensor:
    """(n, present, d) of every record of a four-line FASTQ text: int64 [n_records, 3] on the table's device -- n = the k-mers
    of the record's sequence line; every k-mer has a value, its count c in this table (0: absent; saturated counts as
    stored), taken as 0 when ``c < lower`` (``lower >= 1``); present = the values above 0; d = the value at index
    ``((n - 1) * percentile) // 100`` of the n values in ascending order, 0 when n = 0.  ``percentile`` 50 gives the lower
    median, as ``depth`` does over a packed stream -- the read's depth as BBNorm and khmer's normalize-by-median estimate it;
    0 and 100 give the smallest and the largest value.  Exact for reads of any length.  ``text``, the k-mer rules and the
    errors are those of ``read_hits``.  The table is only read (pg_fastq_index, pg_table_read_depths)."""
    rows = _rows_of_text(self, text, 4, lambda: _depth_args(lower, percentile, min_qual_char),
                         lambda t, n, idx, n_rec, a: _DepthsStep(self, a, bool(lowercase_is_base)).rows(t, n, idx, n_rec, 0))
    return rows[:, :3].contiguous()


# ---------------------------------------------------------------------------------------- files in pieces

class _TableRounds:
    """what ``filter_fastq``, ``trim_fastq``, ``correct_fastq`` and ``normalize_fastq`` do with a round of the piece loop
    (``fastqtext.stream_pieces``): the step's entry on every input and the status read (``check``); the verdicts, the pairing, the
    kept records' sizes and places, their gather and the write (``emit``); the totals -- exact ints, by the places named at this
    module's head -- and the device milliseconds of the timed entries (``result``)"""

    def __init__(self, table, step, pair: str, n_inputs: int):
        self.table, self.step, self.pair = table, step, pair
        self.tot = torch.zeros(N_TOTALS, dtype=torch.int64, device=table.device)
        self.status = torch.empty((n_inputs, 2), dtype=torch.int64, device=table.device)
        self.timed = []                                                  # (event, event) around every timed entry; read at the end
        self.out_dev = None
        self.got = None

    def _events(self) -> tuple:
        self.timed.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        return self.timed[-1]

    def check(self, ins, n):
        self.got = [self.step.launch(s, n, self.status[i], self._events()) for i, s in enumerate(ins)]
        for s, b in zip(ins, self.status[:, 1].cpu().tolist()):
            if b != -1:
                raise ValueError(fastq_error(s.path, b & ((1 << 64) - 1)))

    def emit(self, ins, n, files, writer) -> list:
        step, tot, pair, got = self.step, self.tot, self.pair, self.got
        dev = self.table.device
        passed = []
        for s, rows in zip(ins, got):
            passed.append(step.judge(rows, tot))
            tot[RECORDS] += n
            tot[BASES] += (s.idx[2:4 * n:4] - s.idx[1:4 * n:4] - 1).sum()
        if len(ins) == 2:
            keep = passed[0] | passed[1] if pair == "any" else passed[0] & passed[1]
            keeps = [keep, keep]
        elif pair != "single":
            p2 = passed[0].view(-1, 2)
            keeps = [(p2.any(1) if pair == "any" else p2.all(1)).repeat_interleave(2)]
        else:
            keeps = passed
        taken = []
        for s, keep, f, rows in zip(ins, keeps, files, got):
            kept = keep.nonzero().flatten()
            lens = step.sizes(s, rows, kept, tot)
            dst = torch.cumsum(lens, 0) - lens
            n_kept = int(kept.numel())
            total, used = (int(v) for v in torch.stack([lens.sum(), s.idx[4 * n]]).tolist())
            tot[KEPT] += n_kept
            if total:
                if self.out_dev is None or self.out_dev.numel() < total:
                    self.out_dev = None
                    self.out_dev = torch.empty(total + total // 8, dtype=torch.uint8, device=dev)
                events = self._events()
                events[0].record()
                rc = step.gather(s, n, rows, kept, dst, n_kept, self.out_dev)
                events[1].record()
                _lib.check(rc)
                writer.write(f, self.out_dev, total)
            taken.append(used)
        self.got = None
        return taken

    def result(self) -> tuple:
        totals = self.tot.cpu().tolist()                                 # (a host wait: every timed event has happened)
        return totals, sum(a.elapsed_time(b) for a, b in self.timed)


def _fastq_pieces(table, srcs: list, outs: list, pair: str, step) -> tuple:
    """(totals, device milliseconds) of a verb's files through the piece loop.  An input that carries mates in ONE file needs two
    records to make a round, every other one"""
    table._require_readable()
    mates_in_one = len(srcs) == 1 and pair != "single"
    return fastqtext.stream_pieces(srcs, outs, table.device, _TableRounds(table, step, pair, len(srcs)), pair,
                                   grow_below=2 if mates_in_one else 1)


def correct_fastq(self, src1: str, out1: str, src2: str | None = None, out2: str | None = None, lower: int = 1, upper: int | None = None,
                  lowercase_is_base: bool = True, min_qual_char=None) -> dict:
    """put the single-base substitutions of a FASTQ file's reads right from this table (``read_corrections``) and write EVERY
    record, in input order and with the length it came with, to ``out1`` (and ``out2``): the output is byte for byte the
    input except the corrected bases, so each output has its input's size.  One file (interleaved or not: records are judged
    on their own, an odd number of them is fine) or R1 / R2 (the same number of records).  Input forms, pieces, the plain-text
    output under a temporary name, "after any error no output file is left" and the ValueErrors naming the record's ordinal
    are those of ``trim_fastq``; a quality line that does not reach as far as its sequence line is malformed.

    Returns ``records``, ``bases`` (bytes of the sequence lines), ``kmers``, ``hits`` (of the input), ``candidates``,
    ``corrected``, ``reads_corrected`` (records with at least one corrected base) -- totals over all inputs, exact -- and
    ``seconds`` (wall), ``device_ms`` (the pg_table_correct_reads and pg_fastq_gather entries of every piece, each between
    two device events of its own)."""
    t0 = time.perf_counter()
    pair = "single" if src2 is None else "both"
    srcs, outs = _fastq_files(src1, out1, src2, out2, pair)
    window = _hits_window(lower, upper, min_qual_char)
    totals, device_ms = _fastq_pieces(self, srcs, outs, pair, _CorrectStep(self, window, bool(lowercase_is_base)))
    return {"records": totals[RECORDS], "bases": totals[BASES], "kmers": totals[KMERS], "hits": totals[HITS],
            "candidates": totals[CANDIDATES], "corrected": totals[CORRECTED], "reads_corrected": totals[READS_CORRECTED],
            "seconds": round(time.perf_counter() - t0, 6), "device_ms": round(device_ms, 4)}


def normalize_fastq(self, src1: str, out1: str, src2: str | None = None, out2: str | None = None, target: int | None = None,
                    min_depth: int = 0, lower: int = 1, percentile: int = 50, pair: str = "any", seed: int = 0,
                    lowercase_is_base: bool = True, min_qual_char=None) -> dict:
    """normalise the read depth of a FASTQ file from this table (BBNorm, khmer's normalize-by-median; beside the read set of
    scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp) and write the kept records, byte for byte and in input order, to
    ``out1`` (and ``out2``): what the table covers more than ``target`` deep is thinned to about that depth, what it covers
    less deep passes untouched, and reads whose depth marks them as errors can be dropped.

    The depth d of a record among its n k-mers: ``read_depths`` (``lower``, ``percentile``, ``lowercase_is_base``,
    ``min_qual_char`` as there).  Every unit -- a pair, or a record under ``pair`` "single" -- has ONE draw w in [0, 2^24), a
    function of ``seed`` and the unit's ordinal alone (include/pangaea_feat.h, pg_table_read_depths: DRAW).  A record PASSES
    iff n >= 1, d >= ``min_depth`` and ``w * d < target * 2^24`` (exact integers): with probability ``min(1, target / d)``;
    a read of absent k-mers only has d = 0 and always passes the draw.  ``pair`` as for ``filter_fastq``; mates share their
    draw, so "any" keeps a pair at its smaller depth and "both" at its larger.  ``target``: an int in [1, 2^31);
    ``min_depth``: an int >= 0; ``seed``: an int in [0, 2^64).  The same arguments give the same output whatever the piece
    size.  Input forms, pieces, the plain-text output under a temporary name, "after any error no output file is left" and
    the ValueErrors naming the record's ordinal are those of ``filter_fastq``.

    Returns ``records``, ``kept``, ``passed`` (records that passed on their own), ``low`` (records with n = 0 or
    d < ``min_depth``), ``bases`` (bytes of the sequence lines), ``kmers``, ``hits`` (the sum of present), ``depth_in`` and
    ``depth_out`` (the sum of d over all records and over the kept ones) -- totals over all inputs, exact -- and ``seconds``
    (wall), ``device_ms`` (the pg_table_read_depths and pg_fastq_gather entries of every piece, each between two device
    events of its own)."""
    t0 = time.perf_counter()
    srcs, outs = _fastq_files(src1, out1, src2, out2, pair)
    args = _depth_args(lower, percentile, min_qual_char)
    for name, v, lo, hi in (("target", target, 1, 1 << 31), ("min_depth", min_depth, 0, None), ("seed", seed, 0, 1 << 64)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v >= hi):
            raise ValueError(f"{name} must be an int, at least {lo}" + (f" and below 2^{hi.bit_length() - 1}" if hi else "") + f" (got {v!r})")
    unit_log2 = 1 if len(srcs) == 1 and pair != "single" else 0
    step = _DepthsStep(self, args, bool(lowercase_is_base), int(target), int(min_depth), int(seed), unit_log2)
    totals, device_ms = _fastq_pieces(self, srcs, outs, pair, step)
    return {"records": totals[RECORDS], "kept": totals[KEPT], "passed": totals[PASSED], "low": totals[LOW], "bases": totals[BASES],
            "kmers": totals[KMERS], "hits": totals[HITS], "depth_in": totals[DEPTH_IN], "depth_out": totals[DEPTH_OUT],
            "seconds": round(time.perf_counter() - t0, 6), "device_ms": round(device_ms, 4)}


def filter_fastq(self, src1: str, out1: str, src2: str | None = None, out2: str | None = None, lower: int = 1, upper: int | None = None,
                 min_hits=1, max_hits=None, pair: str = "any", lowercase_is_base: bool = True, min_qual_char=None) -> dict:
    """keep or drop the reads of a FASTQ file by the counts of their k-mers in this table (`kmc_tools filter`, khmer's
    filter-abund; the alignment-free counterpart of scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp) and write the kept
    records, byte for byte and in input order, to ``out1`` (and ``out2``).

    Input: four-line FASTQ, plain or gzip -- one file (``src1``; mates, if any, interleaved) or an R1/R2 pair (``src1``,
    ``src2`` with ``out1``, ``out2``).  Records, k-mers and the hit count h of a read among its n k-mers: ``read_hits``
    (``lower``, ``upper``, ``lowercase_is_base``, ``min_qual_char`` as there).  A read PASSES iff n >= 1, h >= ``min_hits`` and
    h <= ``max_hits``; each bound is an int (absolute) or a float in [0, 1] (a share of n, compared as ``h >= f * n`` /
    ``h <= f * n`` in IEEE double); ``max_hits`` None: no bound.  A read without k-mers never passes.  ``pair``: "any" keeps
    both mates if either passes, "both" if both pass, "single" judges every record on its own (one input file only).  Mates
    are records 2i and 2i + 1 of one file, or record i of R1 and of R2; names are not compared.  ValueError (PG_EFORMAT) with
    the record's ordinal: a first line without ``@``, a third without ``+``, a file that ends inside a record, a short quality
    line under ``min_qual_char``, an odd record count under any / both, R1 / R2 of different record counts.

    Output is plain text (a path ending in ``.gz`` is refused), written under a temporary name of its own beside the output
    and moved into place at the end: after any error no output file is left and no other file has been touched.  The
    outputs must differ from each other and from the inputs.  The files go through the device in pieces of ``FILTER_PIECE_BYTES``
    (PG_FILTER_PIECE_BYTES, read at call time): a piece starts at a record start, what lies behind its last complete record
    (and, for R1 / R2, behind the records both pieces hold) is carried into the next, a record larger than a piece grows the
    buffer.  The device holds one piece per input, its line index, the hits and one output piece.

    Returns ``records``, ``kept``, ``passed`` (records that passed on their own), ``bases`` (bytes of the sequence lines),
    ``kmers``, ``hits`` -- totals over all inputs, exact -- and ``seconds`` (wall), ``device_ms`` (the pg_table_read_hits and
    pg_fastq_gather entries of every piece, each between two device events of its own)."""
    t0 = time.perf_counter()
    srcs, outs = _fastq_files(src1, out1, src2, out2, pair)
    window = _hits_window(lower, upper, min_qual_char)
    lo_bound, hi_bound = _hit_bound(min_hits, "min_hits"), None if max_hits is None else _hit_bound(max_hits, "max_hits")
    totals, device_ms = _fastq_pieces(self, srcs, outs, pair, _HitsStep(self, window, bool(lowercase_is_base), lo_bound, hi_bound))
    return {"records": totals[RECORDS], "kept": totals[KEPT], "passed": totals[PASSED], "bases": totals[BASES], "kmers": totals[KMERS],
            "hits": totals[HITS], "seconds": round(time.perf_counter() - t0, 6), "device_ms": round(device_ms, 4)}


def trim_fastq(self, src1: str, out1: str, src2: str | None = None, out2: str | None = None, lower: int = 1, upper: int | None = None,
               mode: str = "longest", min_len: int | None = None, pair: str = "both", lowercase_is_base: bool = True,
               min_qual_char=None) -> dict:
    """cut the reads of a FASTQ file down to the part this table vouches for (`kmc_tools filter -t`, khmer's filter-abund /
    trim-low-abund; beside the read set of scripts/low_abd_reads.sh:10 -> extract_unmapped.cpp) and write them, in input
    order, to ``out1`` (and ``out2``): a read with one sequencing error keeps its good bases where ``filter_fastq`` could only
    keep the error or drop the read.

    The span of a record -- ``read_spans``: ``mode`` "longest" (the longest run of solid k-mers) or "first" (the read up to its
    first k-mer outside ``[lower, upper]``) -- is (start, length).  A record PASSES iff length >= ``min_len`` (None: k; at
    least 1).  ``pair``: "both" (the default) keeps a pair when both mates pass, "any" when either does, "single" judges every
    record of one file on its own.  EVERY written record is written trimmed to its span: line 0 and line 2 as they are,
    ``seq[start : start + length]`` and ``qual[start : start + length]`` with the line ends they had (``\\r\\n`` stays
    ``\\r\\n``, a final record without ``\\n`` leaves without one); quality bytes beyond the sequence are dropped.  That includes a
    mate kept under "any" that did not pass, possibly with empty sequence and quality lines -- which is why "both" is the
    default here.  A quality line that does not reach as far as its sequence line is malformed, with or without
    ``min_qual_char``.  Input forms, pieces, the plain-text output under a temporary name, "after any error no output file is
    left" and the ValueErrors naming the record's ordinal are those of ``filter_fastq``.

    Returns ``records``, ``kept``, ``passed`` (records that passed on their own), ``trimmed`` (kept records that came out
    shorter than they went in), ``bases`` (bytes of the sequence lines), ``bases_out`` (bases written), ``kmers``, ``hits`` --
    totals over all inputs, exact -- and ``seconds`` (wall), ``device_ms`` (the pg_table_read_spans and
    pg_fastq_gather_trimmed entries of every piece, each between two device events of its own)."""
    t0 = time.perf_counter()
    srcs, outs = _fastq_files(src1, out1, src2, out2, pair)
    window = _hits_window(lower, upper, min_qual_char)
    mode = _span_mode(mode)
    if min_len is None:
        min_len = self.k
    if isinstance(min_len, bool) or not isinstance(min_len, (int, np.integer)) or min_len < 1:
        raise ValueError(f"min_len must be a whole number of bases, at least 1 (got {min_len!r})")
    totals, device_ms = _fastq_pieces(self, srcs, outs, pair, _SpansStep(self, window, bool(lowercase_is_base), mode, int(min_len)))
    return {"records": totals[RECORDS], "kept": totals[KEPT], "passed": totals[PASSED], "trimmed": totals[TRIMMED], "bases": totals[BASES],
            "bases_out": totals[BASES_OUT], "kmers": totals[KMERS], "hits": totals[HITS], "seconds": round(time.perf_counter() - t0, 6),
            "device_ms": round(device_ms, 4)}
