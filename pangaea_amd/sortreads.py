"""Sort the read pairs of a FASTQ file by their barcode on the GPU: what step 0 of the reference's driver does with awk and
``LANG=C sort`` (src/run_pangaea:237-252), as a library call, a command (``pangaea_amd/bin/sort_barcodes``) and a switch of the
orchestrator (``pangaea.py --sort_reads``).  Every entry point of this package takes a barcode-sorted interleaved FASTQ; this
module makes one.

The rule (include/pangaea_feat.h, "Read pairs of a FASTQ text by their barcode tag"):

  unit     a read pair -- 8 lines of an interleaved four-line FASTQ, or record i of ``-1`` with record i of ``-2``
  tag      from the unit's FIRST header only: the leftmost ``BX:Z:`` followed by one or more bytes that are no C-locale white space,
           at its longest; a unit without one is untagged
  order    tagged units by their tag's bytes as unsigned bytes (memcmp, the shorter of two equal prefixes first), untagged
           units behind them; WITHIN one tag the input order (a stable sort) -- the reference's ``sort`` without ``-s`` breaks such
           ties by the whole line (read name, then sequence), an order nothing downstream reads
  output   every unit byte for byte, R1's four lines and then R2's; a last line without ``\\n`` gets one

The whole text lives on the device: the line index (pg_fastq_index), the tags (pg_fastq_barcode_tags), one stable 64-bit
``torch.sort`` per 8-byte chunk of the longest tag over key words made on the device (pg_fastq_tag_keys), the comparison of
neighbours that checks every order before a byte is written (pg_fastq_tag_compare), and the records to their places
(pg_fastq_gather).  A file larger than device memory would need a multi-pass merge: out of scope, refused with the figures.
"""
from __future__ import annotations

import os
import time

import torch

from . import _lib, fastqtext
from .fastqtext import fastq_error, piece_bytes, stream_ptr as _stream_ptr, temp_beside

UNIT_BYTES = 64        # device bytes per unit beside the text: tag_off 8, tag_len 4, compare 1, order, keys and torch.sort's two outputs 8 each
STAGES = ("index", "tags", "sort", "compare", "gather")


def line_index(text: torch.Tensor, n_bytes: int) -> tuple:
    """(line starts: int64 on the text's device, n_lines + 1 entries; n_lines) of text[:n_bytes] -- ``fastqtext.line_index``,
    its buffers cut down to the entries that count"""
    idx, n_lines = fastqtext.line_index(text, n_bytes)
    return idx[:n_lines + 1].clone(), n_lines


def _free_bytes(device) -> int:
    """device bytes a call may still take: what the driver reports free and what torch holds without using it"""
    free, _ = torch.cuda.mem_get_info(device)
    return int(free) + int(torch.cuda.memory_reserved(device)) - int(torch.cuda.memory_allocated(device))


def _require_room(need: int, device, what: str, prepared: bool = False) -> None:
    free = _free_bytes(device)
    if need > free:
        how = ("about 2 x the prepared text's bytes -- the raw reads' and 8 + the barcode's bytes per tagged header -- + 8 per line + 64 per "
               "read pair, and the raw texts with their line indices while the prepared text is made" if prepared
               else "about 2 x its bytes + 8 per line + 64 per read pair")
        raise ValueError(f"{what}: {need} bytes of device memory needed, {free} free -- the whole text is sorted on the device "
                         f"({how}); a multi-pass sort of larger files is not implemented")


def _read_text(path: str, device) -> tuple:
    """(the file's text on the device, its bytes): plain or gzip (told by the first two bytes), staged through one pinned buffer
    of PG_FILTER_PIECE_BYTES; a last line without its newline gets one"""
    f, packed = fastqtext.open_fastq(path)
    piece, size = piece_bytes(), None
    if not packed:
        size = os.path.getsize(path)
        piece = max(64, min(piece, size))
        _require_room(size + size // 2, device, path)          # (the text and its index while that is made)
    host = torch.empty(piece, dtype=torch.uint8, pin_memory=True)
    buf = memoryview(host.numpy())
    text = torch.empty((size if size is not None else piece) + 32, dtype=torch.uint8, device=device)
    n, last = 0, 10
    try:
        while True:
            got = f.readinto(buf)
            if not got:
                break
            if n + got + 32 > text.numel():                              # (gzip, or a file that grew: twice the room)
                _require_room(2 * text.numel(), device, path)
                more = torch.empty(2 * (n + got) + 32, dtype=torch.uint8, device=device)
                more[:n] = text[:n]
                text = more
            text[n:n + got].copy_(host[:got], non_blocking=True)
            torch.cuda.current_stream(device).synchronize()              # (the one pinned buffer is read into again)
            n, last = n + got, buf[got - 1]
    finally:
        f.close()
    if n and last != 10:
        text[n] = 10
        n += 1
    return text, n


def barcode_tags(text: torch.Tensor, idx: torch.Tensor, n_units: int, lines_per_unit: int, n_bytes: int | None = None) -> tuple:
    """(tag_off int64 [n_units], tag_len int32 [n_units], status int64 [2]) of pg_fastq_barcode_tags, on the text's device: the
    byte offset of the ``B`` of each unit's tag (-1: untagged) and the length of the whole match (0); status as
    pg_table_read_hits writes it, the record counted in this text.  ``idx``: the line index, ``lines_per_unit * n_units + 1``
    entries at least."""
    dev = text.device
    n_bytes = int(text.numel()) if n_bytes is None else n_bytes
    if idx.numel() < lines_per_unit * n_units + 1:
        raise ValueError(f"a line index of {idx.numel()} entries does not hold {n_units} units of {lines_per_unit} lines")
    off = torch.empty(n_units, dtype=torch.int64, device=dev)
    length = torch.empty(n_units, dtype=torch.int32, device=dev)
    status = torch.tensor([0, -1], dtype=torch.int64, device=dev)
    if n_units == 0:                                         # (nothing to ask; an empty text has no address to hand over)
        return off, length, status
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pg_fastq_barcode_tags(text.data_ptr(), n_bytes, idx.data_ptr(), n_units, lines_per_unit, off.data_ptr(),
                                                     length.data_ptr(), status.data_ptr(), _stream_ptr(dev)))
    return off, length, status


def tag_keys(text: torch.Tensor, tag_off: torch.Tensor, tag_len: torch.Tensor, order: torch.Tensor | None, byte_begin: int,
             n_bytes: int | None = None) -> torch.Tensor:
    """int64 [n] holding the UNSIGNED key words of pg_fastq_tag_keys: bytes [byte_begin, byte_begin + 8) of the tags behind their
    prefix, big-endian, zero-padded"""
    dev = text.device
    n = int(tag_off.numel())
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    if n == 0:
        return keys
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pg_fastq_tag_keys(text.data_ptr(), int(text.numel()) if n_bytes is None else n_bytes, tag_off.data_ptr(),
                                                 tag_len.data_ptr(), None if order is None else order.data_ptr(), n, byte_begin,
                                                 keys.data_ptr(), _stream_ptr(dev)))
    return keys


def tag_compare(text: torch.Tensor, tag_off: torch.Tensor, tag_len: torch.Tensor, order: torch.Tensor | None = None,
                n_bytes: int | None = None) -> torch.Tensor:
    """int8 [n] of pg_fastq_tag_compare: 0 at 0, else -1 / 0 / +1 as the tag of unit ``order[i - 1]`` stands before, equal to or
    behind that of ``order[i]`` (``order`` None: the identity).  A +1 is a descent; on a sorted order the -1 count the runs."""
    dev = text.device
    n = int(tag_off.numel())
    out = torch.empty(n, dtype=torch.int8, device=dev)
    if n == 0:
        return out
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pg_fastq_tag_compare(text.data_ptr(), int(text.numel()) if n_bytes is None else n_bytes, tag_off.data_ptr(),
                                                    tag_len.data_ptr(), None if order is None else order.data_ptr(), n, out.data_ptr(),
                                                    _stream_ptr(dev)))
    return out


def _order_of(text: torch.Tensor, n_bytes: int, tag_off: torch.Tensor, tag_len: torch.Tensor, longest: int) -> tuple:
    """(the stable order of the units by their tags, passes): one stable sort of 64-bit words per 8-byte chunk of the longest
    tag, from the last chunk to the first (the keys are unsigned: the top bit is flipped for torch's signed sort), then the
    class -- tagged in front of untagged -- as a stable pass of its own, so that no key value stands for "untagged" """
    n = int(tag_off.numel())
    order = torch.arange(n, dtype=torch.int64, device=text.device)
    passes = (longest + 7) // 8
    for chunk in range(passes - 1, -1, -1):
        keys = tag_keys(text, tag_off, tag_len, order, 8 * chunk, n_bytes) ^ (-1 << 63)
        order = order[torch.sort(keys, stable=True).indices]
    tagged = tag_len[order] > 0
    return torch.cat([order[tagged], order[~tagged]]), passes


def barcode_order(text: torch.Tensor, idx: torch.Tensor, n_units: int, lines_per_unit: int) -> torch.Tensor:
    """the permutation that sorts the units of a text by barcode: int64 [n_units] on the text's device, unit ``order[i]`` is the
    i-th of the output.  ValueError for malformed text."""
    off, length, status = barcode_tags(text, idx, n_units, lines_per_unit)
    _raise_malformed("text", status)
    if n_units == 0:
        return torch.zeros(0, dtype=torch.int64, device=text.device)
    longest = max(0, int(length.max().item()) - 5)
    return _order_of(text, int(text.numel()), off, length, longest)[0]


def _status_error(what: str, status: int) -> str:
    if status & 0xFF == _lib.FASTQ_LONG_TAG:
        return f"{what}: record {status >> 8}: its barcode tag is longer than {_lib.FASTQ_MAX_TAG} bytes behind BX:Z: (PG_EFORMAT)"
    return fastq_error(what, status)


def _raise_malformed(what: str, status: torch.Tensor) -> None:
    word = int(status[1].item())
    if word != -1:
        raise ValueError(_status_error(what, word & ((1 << 64) - 1)))


class _Timer:
    """device milliseconds per stage, each stretch between two events of its own"""

    def __init__(self):
        self.spans = []

    def __call__(self, stage: str):
        timer = self

        class _Span:
            def __enter__(self):
                self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                self.a.record()

            def __exit__(self, *exc):
                self.b.record()
                timer.spans.append((stage, self.a, self.b))

        return _Span()

    def result(self) -> dict:
        ms = dict.fromkeys(STAGES, 0.0)
        for stage, a, b in self.spans:
            b.synchronize()
            ms[stage] = ms.get(stage, 0.0) + a.elapsed_time(b)         # (a stage beside STAGES -- prep -- shows only when it ran)
        return {k: round(v, 4) for k, v in ms.items()}


class _Loaded:
    """the input of ``sort_fastq`` / ``check_fastq`` on the device: texts, line indices, the units' tags and what they say"""

    def __init__(self, src1: str, src2: str | None, device, timer: _Timer, reserve_out: bool, short_type=None, index=None):
        self.paths = [os.fspath(src1)] + ([os.fspath(src2)] if src2 is not None else [])
        self.texts, self.sizes, self.idx = [], [], []
        self.lines_per_unit = 8 if src2 is None else 4
        self.prep = None                                     # the counts of the rewriting in front, when there was one
        if short_type is not None:
            if index is not None:
                self.paths.append(os.fspath(index))
            self._prepare(short_type, device, timer, reserve_out)
            src2 = None                                      # (from here on: one interleaved text)
        else:
            self._read(device, timer)
        self._tags(src2, device, timer, reserve_out)

    def _read_indexed(self, path: str, device, timer: _Timer) -> int:
        """one file to the device with its line index; its records"""
        text, n = _read_text(path, device)
        with timer("index"):
            idx, n_lines = line_index(text, n) if n else (torch.zeros(1, dtype=torch.int64, device=device), 0)
        if n_lines % 4:
            raise ValueError(f"{path}: record {n_lines // 4}: the file ends inside it ({n_lines % 4} of its 4 lines) (PG_EFORMAT)")
        self.texts.append(text)
        self.sizes.append(n)
        self.idx.append(idx)
        return n_lines // 4

    def _prepare(self, short_type: str, device, timer: _Timer, reserve_out: bool) -> None:
        """raw stLFR / TELL-seq R1, R2 (and I1) to ONE interleaved text in the BX:Z: form, in input order (prepreads: the plan and
        write kernels); the raw texts are freed, and what follows sees an interleaved input"""
        from . import prepreads
        mode = prepreads._mode(short_type)
        records = [self._read_indexed(path, device, timer) for path in self.paths]
        for path, r in zip(self.paths[1:], records[1:]):
            if r != records[0]:
                raise ValueError(f"{self.paths[0]} holds {records[0]} records, {path} holds {r}: "
                                 "the read files must have the same number of records (PG_EFORMAT)")
        with timer("prep"):
            plan = prepreads.Plan(mode, self.texts, self.sizes, self.idx, records[0])
        error = prepreads.status_error(self.paths, plan.status)
        if error:
            raise ValueError(error)
        with timer("prep"):
            text, n, units = prepreads.interleaved_text(plan, lambda need: _require_room(need, device, self.paths[0], prepared=True))
        flagged = int(plan.tagged.sum().item()) if records[0] else 0
        self.prep = {"short_type": short_type, "raw_pairs": records[0], "prepared_pairs": units, "dropped_pairs": records[0] - units,
                     "tagged_pairs": flagged}
        del plan
        self.texts, self.sizes, self.idx = [text], [n], []   # (the raw texts and their indices are given back here)
        self.lines_per_unit = 8
        _require_room((n if reserve_out else 0) + n // 2, device, self.paths[0], prepared=True)
        with timer("index"):
            idx, n_lines = line_index(text, n) if n else (torch.zeros(1, dtype=torch.int64, device=device), 0)
        if n_lines != 8 * units:
            raise RuntimeError(f"sort_fastq: the prepared text has {n_lines} lines, {8 * units} were written (internal error)")
        self.idx.append(idx)
        self.records = [2 * units]

    def _read(self, device, timer: _Timer) -> None:
        src2 = self.paths[1] if len(self.paths) == 2 else None
        records = []
        for path in self.paths:
            records.append(self._read_indexed(path, device, timer))
        if src2 is None and records[0] % 2:
            raise ValueError(f"{self.paths[0]}: record {records[0] - 1} has no mate: {records[0]} records are an odd number "
                             "(an interleaved file holds records 2i and 2i + 1 as mates; PG_EFORMAT)")
        if src2 is not None and records[0] != records[1]:
            raise ValueError(f"{self.paths[0]} holds {records[0]} records, {self.paths[1]} holds {records[1]}: "
                             "R1 and R2 must have the same number of records (PG_EFORMAT)")
        self.records = records

    def _tags(self, src2, device, timer: _Timer, reserve_out: bool) -> None:
        records = self.records
        self.pairs = records[0] // 2 if src2 is None else records[0]
        self.bytes = sum(self.sizes)
        _require_room((self.bytes if reserve_out else 0) + UNIT_BYTES * self.pairs, device, self.paths[0], self.prep is not None)
        with timer("tags"):
            self.tag_off, self.tag_len, status = barcode_tags(self.texts[0], self.idx[0], self.pairs, self.lines_per_unit, self.sizes[0])
        _raise_malformed(self.paths[0], status)
        if src2 is not None and self.pairs:                  # R2's tags are nobody's business: its two marker bytes alone
            t, ix = self.texts[1], self.idx[1]
            marks = torch.stack([t[ix[0:4 * self.pairs:4]] != ord("@"), t[ix[2:4 * self.pairs:4]] != ord("+")], 1)
            bad = marks.any(1).nonzero().flatten()[:1]
            if bad.numel():
                r = int(bad.item())
                raise ValueError(fastq_error(self.paths[1], r << 8 | (_lib.FASTQ_NO_AT if bool(marks[r, 0]) else _lib.FASTQ_NO_PLUS)))
        if self.pairs:
            self.longest, self.untagged = max(0, int(self.tag_len.max().item()) - 5), int((self.tag_len == 0).sum().item())
        else:
            self.longest = self.untagged = 0

    def compare(self, order, timer: _Timer) -> torch.Tensor:
        with timer("compare"):
            return tag_compare(self.texts[0], self.tag_off, self.tag_len, order, self.sizes[0])

    def barcodes(self, cmp_sorted: torch.Tensor) -> int:
        """distinct tags, from the comparison of a sorted order's neighbours: its runs, less the run of the untagged"""
        if not self.pairs:
            return 0
        return int((cmp_sorted == -1).sum().item()) + 1 - (1 if self.untagged else 0)


def _gather_plan(texts: list, sizes: list, idxs: list, perm: torch.Tensor) -> list:
    """the pg_fastq_gather calls that write the units in the order ``perm``, one per input text: (text, its bytes, its line
    index, its records, kept, dst_off).  One text: its records 2u and 2u + 1 are unit u; two: record u of each, R1's in front."""
    if len(texts) == 1:
        idx = idxs[0]
        kept = torch.stack([2 * perm, 2 * perm + 1], 1).flatten()
        lens = (idx[4::4] - idx[:-4:4])[kept]
        return [(texts[0], sizes[0], idx, int(kept.numel()), kept, torch.cumsum(lens, 0) - lens)]
    len1, len2 = ((ix[4::4] - ix[:-4:4])[perm] for ix in idxs)
    both = len1 + len2
    at1 = torch.cumsum(both, 0) - both
    return [(text, size, ix, int(perm.numel()), perm, dst) for text, size, ix, dst in zip(texts, sizes, idxs, (at1, at1 + len1))]


def _gather_run(plan: list, out_dev: torch.Tensor, out_bytes: int) -> None:
    lib = _lib.load()
    for text, size, idx, n_records, kept, dst in plan:
        _lib.check(lib.pg_fastq_gather(text.data_ptr(), size, idx.data_ptr(), n_records, kept.data_ptr(), dst.data_ptr(), int(kept.numel()),
                                       out_dev.data_ptr(), out_bytes, _stream_ptr(text.device)))


def _short_type_of(short_type, src1, src2, index, outs: list):
    """``short_type`` as ``_Loaded`` takes it: None for barcodes that stand in a BX:Z: tag already (None, "10x"), else stlfr /
    tellseq with their files checked (ValueError)"""
    if short_type is None or short_type == "10x":
        if index is not None:
            raise ValueError(f"index reads go with short_type tellseq only, not with {short_type or '10x'}")
        return None
    from . import prepreads
    if short_type not in prepreads.SHORT_TYPES:
        raise ValueError(f"short_type must be 10x, stlfr or tellseq (got {short_type!r})")
    if src2 is None:
        raise ValueError(f"{short_type} reads are given as -1 R1 -2 R2, not interleaved: the barcode of a pair is rewritten on both mates")
    prepreads.check_files(short_type, src1, src2, index, outs)
    return short_type


def sort_fastq(src1: str, out: str, src2: str | None = None, device=None, short_type: str | None = None, index: str | None = None) -> dict:
    """write the read pairs of ``src1`` (interleaved) or of ``src1`` / ``src2`` (R1 / R2), plain or gzip, to ``out`` as one
    interleaved plain FASTQ sorted by barcode: the rule of this module's head.  The output is written under a temporary name
    beside ``out`` and moved into place at the end.  ValueError with the record's ordinal: a header without ``@``, a third line
    without ``+``, a file that ends inside a record, an odd record count in an interleaved file, R1 / R2 of different record
    counts, a tag of more than 255 bytes behind ``BX:Z:``; and for an input that does not fit the device, with the bytes needed
    and free.  Every order is checked by pg_fastq_tag_compare before a byte is written (a descent raises RuntimeError).

    Returns ``pairs``, ``barcodes`` (distinct tags), ``untagged_pairs``, ``longest_tag`` (bytes behind the prefix), ``passes``
    (sorts run: 0 when ``already_sorted``), ``already_sorted`` (the input's own order has no descent: it is copied), ``bytes``
    (written), ``seconds`` (wall) and ``device_ms`` per stage -- index, tags, sort (keys + sorts), compare, gather.

    ``short_type`` "stlfr" or "tellseq" (``-1``/``-2`` only; ``index``: TELL-seq's index reads): the inputs are RAW reads, rewritten
    first as ``prepreads.preprocess_reads`` rewrites them, on the device and in input order, into one interleaved text that then
    goes through everything above unchanged -- one more pass over the text than an order made from the raw barcodes would need,
    by code that is pinned already.  Needs about 2 x the prepared text on the device, and the raw texts while it is made.  The
    result then also holds ``short_type``, ``raw_pairs``, ``prepared_pairs``, ``dropped_pairs`` (TELL-seq: index reads that are not
    18 bytes), ``tagged_pairs`` and a ``prep`` entry in ``device_ms``.  None or "10x": nothing changes."""
    t0 = time.perf_counter()
    dev = fastqtext.device_of(device, "sorting reads by barcode")
    out = os.fspath(out)
    if out.endswith(".gz"):
        raise ValueError(f"{out}: the sorted reads are written as plain text, gzip output is not supported")
    if os.path.realpath(out) in {os.path.realpath(os.fspath(p)) for p in (src1, src2, index) if p is not None}:
        raise ValueError(f"the output must differ from the inputs (got {out})")
    short_type = _short_type_of(short_type, src1, src2, index, [out])
    timer = _Timer()
    with torch.cuda.device(dev):
        L = _Loaded(src1, src2, dev, timer, reserve_out=True, short_type=short_type, index=index)
        n, passes = L.pairs, 0
        order, sorted_in = None, True
        if n:
            sorted_in = not bool((L.compare(None, timer) == 1).any().item())
            if not sorted_in:
                with timer("sort"):
                    order, passes = _order_of(L.texts[0], L.sizes[0], L.tag_off, L.tag_len, L.longest)
            cmp_sorted = L.compare(order, timer)
            if bool((cmp_sorted == 1).any().item()):
                raise RuntimeError("sort_fastq: the order made of the key words has a descent under pg_fastq_tag_compare (internal error)")
            barcodes = L.barcodes(cmp_sorted)
            perm = torch.arange(n, dtype=torch.int64, device=dev) if order is None else order
            out_dev = torch.empty(L.bytes + 16, dtype=torch.uint8, device=dev)
            with timer("gather"):
                _gather_run(_gather_plan(L.texts, L.sizes, L.idx, perm), out_dev, L.bytes)
        else:
            barcodes, out_dev = 0, None
        f, tmp = temp_beside(out)
        try:
            if L.bytes:
                piece = max(64, min(piece_bytes(), L.bytes))
                writer = fastqtext.PinnedWriter(dev, piece)
                for at in range(0, L.bytes, piece):
                    m = min(piece, L.bytes - at)
                    writer.write(f, out_dev[at:at + m], m)
            f.close()
            os.replace(tmp, out)
        finally:
            f.close()
            if os.path.exists(tmp):
                os.remove(tmp)
        device_ms = timer.result()
    res = {"pairs": n, "barcodes": barcodes, "untagged_pairs": L.untagged, "longest_tag": L.longest, "passes": passes,
           "already_sorted": sorted_in, "bytes": L.bytes, "seconds": round(time.perf_counter() - t0, 6), "device_ms": device_ms}
    if L.prep is not None:
        device_ms.setdefault("prep", 0.0)
        res.update(L.prep)
    return res


def check_fastq(src1: str, src2: str | None = None, device=None, short_type: str | None = None, index: str | None = None) -> dict:
    """is the input sorted by barcode as ``sort_fastq`` sorts?  ``sorted``; ``first_descent``: the ordinal of the first unit whose
    tag stands before its predecessor's, or None; ``pairs``, ``barcodes`` (distinct tags: an unsorted input is ordered, not
    written, to count them), ``untagged_pairs``.  The refusals are ``sort_fastq``'s.  ``short_type`` / ``index`` as there: the
    question is asked of the raw reads as they would be prepared (ordinals count the prepared units), and the preprocess
    counts are in the result."""
    dev = fastqtext.device_of(device, "sorting reads by barcode")
    short_type = _short_type_of(short_type, src1, src2, index, [])
    timer = _Timer()
    with torch.cuda.device(dev):
        L = _Loaded(src1, src2, dev, timer, reserve_out=False, short_type=short_type, index=index)
        first = None
        cmp_sorted = None
        if L.pairs:
            cmp_in = L.compare(None, timer)
            down = (cmp_in == 1).nonzero().flatten()[:1]
            if down.numel():
                first = int(down.item())
                cmp_sorted = L.compare(_order_of(L.texts[0], L.sizes[0], L.tag_off, L.tag_len, L.longest)[0], timer)
            else:
                cmp_sorted = cmp_in
        res = {"sorted": first is None, "first_descent": first, "pairs": L.pairs, "barcodes": L.barcodes(cmp_sorted) if L.pairs else 0,
               "untagged_pairs": L.untagged}
        if L.prep is not None:
            res.update(L.prep)
        return res
