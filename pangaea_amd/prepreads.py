"""Raw stLFR and TELL-seq read pairs brought to the form every entry point of this package takes -- the barcode in a ``BX:Z:``
tag on both mates' headers -- on the GPU: what the first half of step 0 of the reference's driver does with ``preprocess_stlfr
-n -l`` (src/run_pangaea:138-149, preprocess_stlfr.cpp:68-113) and ``preprocess_tellseq -l INDEX`` (src/run_pangaea:151-162,
preprocess_tellseq.cpp:52-84), as a library call and a command (``pangaea_amd/bin/preprocess_reads``).  ``sortreads.sort_fastq`` /
``check_fastq`` take the same rewriting in front of the sort (``short_type=``), so that raw R1 / R2 (and I1) become the sorted
interleaved file in one call.

The rules (include/pangaea_feat.h, "Raw stLFR and TELL-seq read pairs brought to the BX:Z: form"; bytes, a line's content is the
line without its ``\\n``, ``\\r`` is an ordinary byte; h = the content of R1's header):

  stlfr    p = the first ``#`` in h, q = the first ``/`` behind it or the end, B = h[p + 1 : q], split at its first two ``_`` into
           f1, f2 and the rest.  Tagged iff f1 != "0" and f2 != "0" -- the reference tests f1 twice and never the third field
           (preprocess_stlfr.cpp:89), so ``5_6_0`` is tagged and ``5_0_7``, ``0_6_7``, ``0_0_0`` are not; kept exactly so.  Both
           mates' new header is h[:p], then ``\\tBX:Z:`` + B + ``-1`` if tagged; R2's own header is discarded.  Lines 1 .. 3 of
           each mate byte for byte.  No unit is dropped.
  tellseq  B = the content of the sequence line of the index read.  Kept iff B has exactly 18 bytes (18 + ``\\r`` is 19: dropped,
           counted, no error).  s = the first space in h or its end (a tab does not cut).  Both mates' new header is h[:s] +
           ``\\tBX:Z:`` + B + ``-1``; line 1 byte for byte, line 2 becomes ``+``, line 3 byte for byte.  ``PREFIX.wl`` holds B per
           kept unit, in input order.
  both     a last line without ``\\n`` gets one.  Refused with the record's ordinal (ValueError): a header without ``@`` or a third
           line without ``+`` in any of the files, a file that ends inside a record, files of different record counts, a stLFR
           header without ``#`` or with fewer than two ``_`` in B, a B of more than 253 bytes.  The reference checks none of this:
           parity is claimed on well-formed input only.

The plan of a text (pg_fastq_prep_plan: where the barcode lies, tagged / kept, the status words) and the writing of the new
records to scanned places (pg_fastq_prep_write: both mates, two buffers or one interleaved) are HIP kernels; the lengths between
them are element-wise arithmetic on the line indices and the plan arrays and one ``torch.cumsum``."""
from __future__ import annotations

import os
import time

import torch

from . import _lib, fastqtext
from .fastqtext import fastq_error, stream_ptr as _stream_ptr

SHORT_TYPES = ("stlfr", "tellseq")


def _mode(short_type: str) -> int:
    if short_type not in _lib.PREP_MODES:
        raise ValueError(f"short_type must be stlfr or tellseq (got {short_type!r})")
    return _lib.PREP_MODES[short_type]


def status_error(paths: list, status: torch.Tensor):
    """the message for the status rows of pg_fastq_prep_plan (one per file), or None: the malformed record with the smallest
    ordinal, of the first file that has it"""
    words = [w & ((1 << 64) - 1) for w in status.view(-1, 2)[:len(paths), 1].cpu().tolist()]
    bad = [(w >> 8, f) for f, w in enumerate(words) if w != _lib.FASTQ_CLEAN]
    if not bad:
        return None
    record, f = min(bad)
    reason = words[f] & 0xFF
    why = {_lib.FASTQ_NO_HASH: "its header holds no '#' in front of a stLFR barcode",
           _lib.FASTQ_FEW_FIELDS: "its stLFR barcode holds fewer than two '_'",
           _lib.FASTQ_LONG_TAG: f"its barcode is longer than {_lib.FASTQ_MAX_TAG - 2} bytes"}.get(reason)
    if why is None:
        return fastq_error(paths[f], words[f])
    return f"{paths[f]}: record {record}: {why} (PG_EFORMAT)"


class Plan:
    """what pg_fastq_prep_plan says of the units of a text: head_len int64, bc_off int64, bc_len int32, tagged uint8 (all
    [n_units], on the texts' device) and the status rows int64 [3][2]"""

    def __init__(self, mode: int, texts: list, sizes: list, idxs: list, n_units: int, first_unit: int = 0):
        dev = texts[0].device
        self.mode, self.texts, self.sizes, self.idxs, self.n = mode, texts, sizes, idxs, n_units
        self.head_len = torch.empty(n_units, dtype=torch.int64, device=dev)
        self.bc_off = torch.empty(n_units, dtype=torch.int64, device=dev)
        self.bc_len = torch.empty(n_units, dtype=torch.int32, device=dev)
        self.tagged = torch.empty(n_units, dtype=torch.uint8, device=dev)
        self.status = torch.tensor([[0, -1]] * 3, dtype=torch.int64, device=dev)
        want = 3 if mode == _lib.PREP_TELLSEQ else 2
        if len(texts) != want or len(sizes) != want or len(idxs) != want:
            raise ValueError(f"{want} texts with their sizes and line indices are needed (got {len(texts)})")
        for ix in idxs:
            if ix.numel() < 4 * n_units + 1:
                raise ValueError(f"a line index of {ix.numel()} entries does not hold {n_units} records of 4 lines")
        if n_units == 0:                                     # (nothing to ask; an empty text has no address to hand over)
            return
        third = (texts[2].data_ptr(), sizes[2], idxs[2].data_ptr()) if want == 3 else (None, 0, None)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pg_fastq_prep_plan(mode, texts[0].data_ptr(), sizes[0], idxs[0].data_ptr(), texts[1].data_ptr(), sizes[1],
                                                      idxs[1].data_ptr(), *third, n_units, first_unit, self.head_len.data_ptr(),
                                                      self.bc_off.data_ptr(), self.bc_len.data_ptr(), self.tagged.data_ptr(),
                                                      self.status.data_ptr(), _stream_ptr(dev)))

    def kept(self):
        """the units that are written, int64 ordinals: None for every unit (stLFR), the kept ones for TELL-seq"""
        return self.tagged.nonzero().flatten() if self.mode == _lib.PREP_TELLSEQ else None

    def record_bytes(self, kept) -> tuple:
        """(bytes of R1's new records, of R2's) of the units ``kept`` (None: all), int64: the new header and its '\\n', the rest of
        the mate's own record (TELL-seq: line 1, ``+\\n``, line 3), one more for a record that lacks its final newline"""
        header = self.head_len + self.tagged.to(torch.int64) * (8 + self.bc_len.to(torch.int64)) + 1
        out = []
        for text, size, ix in zip(self.texts[:2], self.sizes[:2], self.idxs[:2]):
            s1, s2, s3, s4 = (ix[k:4 * self.n + k:4] for k in (1, 2, 3, 4))
            rest = (s2 - s1) + 2 + (s4 - s3) if self.mode == _lib.PREP_TELLSEQ else s4 - s1
            lens = header + rest
            if self.n and size and int(text[size - 1].item()) != 10:         # (only the text's last record can lack its newline)
                lens[-1] += 1
            out.append(lens if kept is None else lens[kept])
        return out[0], out[1]

    def write(self, kept, dst1: torch.Tensor, dst2: torch.Tensor, out1: torch.Tensor, out1_bytes: int, out2: torch.Tensor, out2_bytes: int,
              white_list: torch.Tensor | None = None) -> None:
        n_kept = self.n if kept is None else int(kept.numel())
        if n_kept == 0:
            return
        dev = self.texts[0].device
        third = (self.texts[2].data_ptr(), self.sizes[2]) if self.mode == _lib.PREP_TELLSEQ else (None, 0)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().pg_fastq_prep_write(self.mode, self.texts[0].data_ptr(), self.sizes[0], self.idxs[0].data_ptr(),
                                                       self.texts[1].data_ptr(), self.sizes[1], self.idxs[1].data_ptr(), *third, self.n,
                                                       self.head_len.data_ptr(), self.bc_off.data_ptr(), self.bc_len.data_ptr(),
                                                       self.tagged.data_ptr(), None if kept is None else kept.data_ptr(), dst1.data_ptr(),
                                                       dst2.data_ptr(), n_kept, out1.data_ptr(), out1_bytes, out2.data_ptr(), out2_bytes,
                                                       None if white_list is None else white_list.data_ptr(),
                                                       0 if white_list is None else int(white_list.numel()), _stream_ptr(dev)))


def interleaved_text(plan: Plan, before_alloc=None) -> tuple:
    """(the new records of a plan's kept units as ONE interleaved text on the device -- R1's record, then R2's, unit by unit, what
    ``seqtk mergepe`` makes of the two files, src/run_pangaea:224 --, its bytes, the units in it).  ``before_alloc(bytes)`` is
    called with the text's size before it is allocated (the caller's memory check)."""
    dev = plan.texts[0].device
    kept = plan.kept()
    len1, len2 = plan.record_bytes(kept)
    both = len1 + len2
    at1 = torch.cumsum(both, 0) - both
    n_bytes = int(both.sum().item())
    if before_alloc is not None:
        before_alloc(n_bytes + 32)
    out = torch.empty(n_bytes + 32, dtype=torch.uint8, device=dev)
    plan.write(kept, at1, at1 + len1, out, n_bytes, out, n_bytes)
    return out, n_bytes, int(both.numel())


def check_files(short_type, reads1, reads2, index, outs: list) -> list:
    """the input paths of a call, refused before anything is opened where they make no sense (ValueError)"""
    if short_type not in SHORT_TYPES:
        raise ValueError(f"short_type must be stlfr or tellseq (got {short_type!r})")
    if not reads1 or not reads2:
        raise ValueError(f"{short_type} reads are given as -1 R1 -2 R2: the barcode of a pair is rewritten on both mates")
    if short_type == "tellseq" and not index:
        raise ValueError("tellseq reads need their index reads (-I INDEX): the barcode stands there")
    if short_type != "tellseq" and index:
        raise ValueError(f"index reads (-I) go with tellseq only, not with {short_type}")
    srcs = [os.fspath(reads1), os.fspath(reads2)] + ([os.fspath(index)] if index else [])
    fastqtext.check_outputs(outs, srcs, "the reads")
    return srcs


class _PrepRounds:
    """what ``preprocess_reads`` does with a round of the piece loop (``fastqtext.stream_pieces``): the plan of the round's units and
    its status rows (``check``); the new records' lengths, their scan, the write kernel and the bytes to the files (``emit``); the
    counts and the device milliseconds per stage (``result``)"""

    def __init__(self, mode: int, srcs: list, device):
        self.mode, self.srcs, self.device = mode, srcs, device
        self.pairs = self.flagged = self.bytes = 0
        self.timed = {"index": [], "plan": [], "write": []}
        self.plan = self.used = None

    def _span(self, stage):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.timed[stage].append((a, b))
        a.record()
        return b

    def check(self, ins, n):
        self.used = [int(v) for v in torch.stack([s.idx[4 * n] for s in ins]).tolist()]
        end = self._span("plan")
        self.plan = Plan(self.mode, [s.text for s in ins], self.used, [s.idx for s in ins], n, self.pairs)
        end.record()
        error = status_error(self.srcs, self.plan.status)
        if error:
            raise ValueError(error)

    def emit(self, ins, n, files, writer) -> list:
        plan, dev, tellseq = self.plan, self.device, self.mode == _lib.PREP_TELLSEQ
        end = self._span("write")
        kept = plan.kept()
        len1, len2 = plan.record_bytes(kept)
        n1, n2 = (int(v) for v in torch.stack([len1.sum(), len2.sum()]).tolist())
        n_kept = int(len1.numel())
        out1 = torch.empty(n1 + 32, dtype=torch.uint8, device=dev)
        out2 = torch.empty(n2 + 32, dtype=torch.uint8, device=dev)
        wl = torch.empty(19 * n_kept, dtype=torch.uint8, device=dev) if tellseq and n_kept else None
        plan.write(kept, torch.cumsum(len1, 0) - len1, torch.cumsum(len2, 0) - len2, out1, n1, out2, n2, wl)
        end.record()
        for f, buf, m in zip(files, (out1, out2, wl), (n1, n2, 19 * n_kept)):
            if buf is None or not m:
                continue
            writer.write(f, buf, m)
            self.bytes += m
        self.pairs += n
        self.flagged += int(plan.tagged.sum().item())
        self.plan = None
        return self.used

    def result(self) -> dict:
        torch.cuda.current_stream(self.device).synchronize()
        return {k: round(sum(a.elapsed_time(b) for a, b in v), 4) for k, v in self.timed.items()}


def preprocess_reads(short_type: str, reads1: str, reads2: str, out_prefix: str, index: str | None = None, device=None) -> dict:
    """write ``out_prefix_1.fq`` and ``out_prefix_2.fq`` (and ``out_prefix.wl`` for TELL-seq: the reference tools' file names) from
    raw R1 / R2 (and the index reads I1), plain or gzip, by the rules of this module's head.  Files of any size: the inputs are
    read in pieces of PG_FILTER_PIECE_BYTES (read at call time); a round takes the records every input holds whole, so inputs
    whose records differ in length stay aligned by record ordinal.  The outputs are plain text, written under temporary names
    and moved into place at the end.

    Returns ``short_type``, ``pairs`` (read), ``tagged_pairs`` and ``untagged_pairs`` (stLFR; all are written) or ``kept_pairs``
    and ``dropped_pairs`` (TELL-seq), ``bytes`` (written, all files), ``files``, ``seconds`` (wall) and ``device_ms`` per stage --
    index, plan, write (the lengths and their scan included)."""
    t0 = time.perf_counter()
    mode = _mode(short_type)
    prefix = os.fspath(out_prefix)
    outs = [prefix + "_1.fq", prefix + "_2.fq"] + ([prefix + ".wl"] if mode == _lib.PREP_TELLSEQ else [])
    srcs = check_files(short_type, reads1, reads2, index, outs)
    dev = fastqtext.device_of(device, "preprocessing reads")
    rounds = _PrepRounds(mode, srcs, dev)
    device_ms = fastqtext.stream_pieces(srcs, outs, dev, rounds, pair=None, grow_below=1, index_events=rounds.timed["index"])
    pairs, flagged = rounds.pairs, rounds.flagged
    counts = ({"kept_pairs": flagged, "dropped_pairs": pairs - flagged} if mode == _lib.PREP_TELLSEQ
              else {"tagged_pairs": flagged, "untagged_pairs": pairs - flagged})
    return {"short_type": short_type, "pairs": pairs, **counts, "bytes": rounds.bytes, "files": outs,
            "seconds": round(time.perf_counter() - t0, 6), "device_ms": device_ms}
