"""Four-line FASTQ text on the device: what every read-processing verb of this package shares, and nothing of k-mer tables.  A
file goes through the device in pieces (``FastqPieces``: the pinned buffer, the piece on the device, its line index --
pg_fastq_index); ``take_round`` says how many records a round takes of its inputs and what error is pending; ``stream_pieces`` is
the ONE piece loop -- inputs, temporary outputs, rounds, growth, the end, the move into place, the cleanup -- and its clients
(``readops``: filter / trim / correct / normalize; ``prepreads.preprocess_reads``) supply what a round checks and writes.
``sortreads`` keeps its whole text on the device and takes the line index, the gzip sniff and the pinned write-out from here."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

PIECE_BYTES = 256 << 20                # FASTQ text per piece and input (device buffer + pinned host buffer)


def piece_bytes() -> int:
    """PG_FILTER_PIECE_BYTES overrides the piece size (tests: records across every boundary, a record larger than a piece)"""
    want = os.environ.get("PG_FILTER_PIECE_BYTES")
    return max(64, int(want)) if want else PIECE_BYTES


def stream_ptr(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def device_of(device, what: str):
    """the device of a call that names none or leaves its ordinal open; ``what`` needs a GPU"""
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs a GPU: the kernels have no CPU path")
    dev = torch.device("cuda") if device is None else torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def line_index(text: torch.Tensor, n_bytes: int, hold: dict | None = None) -> tuple:
    """(line starts: int64 on the text's device, entries 0 .. n_lines valid; n_lines) of text[:n_bytes] (pg_fastq_index).  ``hold``
    keeps the index buffer and the workspace for the next piece.  A host wait."""
    L = _lib.load()
    dev = text.device
    hold = {} if hold is None else hold
    need = _lib.check(L.pg_fastq_index_workspace_bytes(n_bytes))
    if hold.get("ws") is None or hold["ws"].numel() < need:
        hold["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    cap = n_bytes // 16 + 1024               # (reads have lines of 50 bytes and more; a text of shorter ones asks twice)
    while True:
        if hold.get("idx") is None or hold["idx"].numel() < cap:
            hold["idx"] = torch.empty(cap, dtype=torch.int64, device=dev)
        idx = hold["idx"]
        _lib.check(L.pg_fastq_index(text.data_ptr(), n_bytes, idx.data_ptr(), idx.numel(), word.data_ptr(), hold["ws"].data_ptr(),
                                    hold["ws"].numel(), stream_ptr(dev)))
        n_lines = int(word.item())
        if n_lines + 1 <= idx.numel():
            return idx, n_lines
        cap = n_lines + 1


def fastq_error(what: str, status: int) -> str:
    """the message for status[1] of pg_table_read_hits: the malformed record with the smallest ordinal, and why"""
    record, reason = status >> 8, status & 0xFF
    why = {_lib.FASTQ_NO_AT: "its first line does not begin with '@'", _lib.FASTQ_NO_PLUS: "its third line does not begin with '+'",
           _lib.FASTQ_SHORT_QUALITY: "its quality line is shorter than its sequence line",
           _lib.FASTQ_BAD_INDEX: "the line index does not describe the text"}.get(reason, f"reason {reason}")
    return f"{what}: record {record}: {why} (PG_EFORMAT)"


def check_outputs(outs: list, srcs: list, noun: str) -> None:
    """the output paths of a call, refused before anything is opened (ValueError): ``noun`` are written as plain text, to files
    that differ from each other and from the inputs"""
    for o in outs:
        if o.endswith(".gz"):
            raise ValueError(f"{o}: {noun} are written as plain text, gzip output is not supported")
    real_outs = [os.path.realpath(x) for x in outs]
    if len(set(real_outs)) != len(outs) or set(real_outs) & {os.path.realpath(x) for x in srcs}:
        raise ValueError("the outputs must differ from each other and from the inputs (got " + ", ".join(outs + srcs) + ")")


def temp_beside(path: str) -> tuple:
    """(file open for writing, its name): a new file of a name nobody else has, in the directory of ``path`` (so that it can be
    moved into place), with the mode a plain ``open`` would have given it"""
    import tempfile
    fd, tmp = tempfile.mkstemp(dir=os.path.dirname(os.path.abspath(path)), prefix=os.path.basename(path) + ".", suffix=".tmp")
    mask = os.umask(0)
    os.umask(mask)
    os.chmod(tmp, 0o666 & ~mask)
    return os.fdopen(fd, "wb"), tmp


def open_fastq(path: str) -> tuple:
    """(the file open for reading bytes, is it gzip): plain (unbuffered) or gzip, told by the first two bytes"""
    with open(path, "rb") as probe:
        packed = probe.read(2) == b"\x1f\x8b"
    if packed:
        import gzip
        return gzip.open(path, "rb"), True
    return open(path, "rb", buffering=0), False


class PinnedWriter:
    """device bytes to a file through ONE pinned staging buffer: of ``size`` bytes from the start, or (None) grown to m + m // 8
    when a write of m bytes asks for more than it has"""

    def __init__(self, device, size: int | None = None):
        self.device = device
        self.host = None if size is None else torch.empty(size, dtype=torch.uint8, pin_memory=True)

    def write(self, f, buf: torch.Tensor, m: int) -> None:
        """bytes [0, m) of ``buf`` to ``f``.  A host wait."""
        if self.host is None or self.host.numel() < m:
            self.host = None
            self.host = torch.empty(m + m // 8, dtype=torch.uint8, pin_memory=True)
        self.host[:m].copy_(buf[:m], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        f.write(memoryview(self.host.numpy())[:m])


def take_round(ins: list, pair) -> tuple:
    """what one round takes of its indexed pieces: (records per input, the error that ends the call once those records are found
    well-formed or None, every input has ended).  The records are the whole ones every piece holds.  ``pair`` is the caller's
    flavour: "any" / "both" / "single" for the verbs of a table (one file, or R1 / R2), None for N files aligned by record ordinal
    (preprocess).  Under any / both the records of ONE file are mates 2i and 2i + 1: an even number of them while the file goes
    on, and an odd count at its end is an error.  Pending errors beside that: an input that ends inside a record; one that ends at
    a record boundary while another holds more.  Where one input ends at a boundary and another inside that very record, the
    table verbs name the count mismatch and preprocess the torn record."""
    n = min(s.n_rec for s in ins)
    all_eof = all(s.eof for s in ins)
    noun = "the read files" if pair is None else "R1 and R2"
    uneven = torn = None
    for s in ins:
        for o in ins:
            if uneven is None and o is not s and s.eof and s.n_rec == n and not s.n_lines % 4 and (o.n_rec > n or (o.eof and o.n_lines > 4 * n)):
                uneven = f"{s.path} ends after {s.done + n} records, {o.path} holds more: {noun} must have the same number of records (PG_EFORMAT)"
    for s in ins:
        if torn is None and s.eof and s.n_rec == n and s.n_lines % 4:
            torn = f"{s.path}: record {s.done + n}: the file ends inside it ({s.n_lines % 4} of its 4 lines) (PG_EFORMAT)"
    pending = (torn or uneven) if pair is None else (uneven or torn)
    if len(ins) == 1 and pair in ("any", "both") and n & 1:
        if all_eof:
            pending = pending or (f"{ins[0].path}: record {ins[0].done + n - 1} has no mate: {ins[0].done + n} records are an odd number "
                                  f"(pair={pair!r} takes records 2i and 2i + 1 as mates; PG_EFORMAT)")
        else:
            n -= 1
    return n, pending, all_eof


class FastqPieces:
    """one input of the piece loop: the file (plain or gzip), the pinned buffer its pieces are read into, the piece on the device
    and its line index.  The buffers are no larger than the input asks: a plain file's size is known, a gzip file's buffer starts
    at ``START`` bytes and doubles up to the piece while the file goes on"""
    START = 1 << 20

    def __init__(self, path: str, piece: int, device):
        self.path, self.device = path, device
        self.f, packed = open_fastq(path)
        if packed:
            self.limit, piece = piece, min(piece, self.START)
        else:
            piece = max(64, min(piece, os.path.getsize(path) + 1))       # (a small file: one piece of its own size, and the end seen at once)
            self.limit = piece
        self.cap = piece
        self.host = torch.empty(piece, dtype=torch.uint8, pin_memory=True)
        self.buf = self.host.numpy()
        self.text = None
        self.have, self.eof, self.done = 0, False, 0     # bytes in the buffer, the file has ended, records of earlier pieces
        self.hold = {}
        self.idx, self.n_lines, self.n_rec = None, 0, 0

    def fill(self) -> None:
        while not self.eof:
            if self.have == self.cap:
                if self.cap >= self.limit:
                    break
                self._resize(min(2 * self.cap, self.limit))          # (a buffer that began small: up to the piece)
            got = self.f.readinto(memoryview(self.buf)[self.have:self.cap])
            if not got:
                self.eof = True
            else:
                self.have += got

    def _resize(self, cap: int) -> None:
        host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        host[:self.have] = self.host[:self.have]
        self.cap, self.host, self.buf = cap, host, host.numpy()

    def grow(self) -> None:
        """twice the piece: a record (a pair of them) that no piece holds"""
        self.limit = 2 * self.cap
        self._resize(self.limit)

    def index(self) -> None:
        """the piece to the device, its lines counted and indexed; n_rec = the records that are whole (before the end of the file
        a line without its newline is not yet a line)"""
        if self.have == 0:
            self.n_lines = self.n_rec = 0
            return
        if self.text is None or self.text.numel() < self.cap + 16:
            self.text = None
            self.text = torch.empty(self.cap + 16, dtype=torch.uint8, device=self.device)
        self.text[:self.have].copy_(self.host[:self.have], non_blocking=True)
        self.idx, self.n_lines = line_index(self.text, self.have, self.hold)
        whole = self.n_lines if self.eof else self.n_lines - int(self.buf[self.have - 1] != 10)
        self.n_rec = whole // 4

    def consume(self, used: int, n_records: int) -> None:
        """the first ``used`` bytes (``n_records`` records) are dealt with: what lies behind them moves to the front"""
        rest = self.have - used
        if rest:
            self.buf[:rest] = self.buf[used:self.have].copy()
        self.have, self.done = rest, self.done + n_records

    def close(self) -> None:
        if self.f is not None:
            self.f.close()
            self.f = None


def stream_pieces(srcs: list, outs: list, device, client, pair, grow_below: int, index_events: list | None = None):
    """the piece loop: the inputs ``srcs`` go through the device in pieces of ``piece_bytes()``, round by round, and ``outs`` are
    written under temporary names and moved into place at the end; after any error no output file is left and no other file has
    been touched.  A round takes the records ``take_round(ins, pair)`` gives; an input that holds fewer than ``grow_below``
    records while nothing can be taken gets a longer buffer.  ``index_events``: a list that receives one pair of device events
    per round, recorded around the pieces' way to the device and their line indices (None: not timed).

    ``client`` is what a verb does with a round of ``n`` records of each of ``ins``:
      ``check(ins, n)``                 runs right after the round is taken: it enqueues what reads the records and raises
                                        ValueError for a malformed one -- the malformed record in front comes before what is pending
      ``emit(ins, n, files, writer)``   writes the round's bytes to the open outputs (``writer``: a ``PinnedWriter``) and returns the
                                        bytes of each input that the n records took
      ``result()``                      what the call returns, asked once behind the last round and before the outputs are moved"""
    piece = piece_bytes()
    ins, files, tmps = [], [], []
    try:
        with torch.cuda.device(device):
            for path in srcs:
                ins.append(FastqPieces(path, piece, device))
            for o in outs:
                f, tmp = temp_beside(o)
                files.append(f)
                tmps.append(tmp)
            writer = PinnedWriter(device)
            done = False
            while not done:
                for s in ins:
                    s.fill()
                if index_events is not None:
                    index_events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                    index_events[-1][0].record()
                for s in ins:
                    s.index()
                if index_events is not None:
                    index_events[-1][1].record()
                n, pending, all_eof = take_round(ins, pair)
                if n == 0 and pending is None and not all_eof:           # a buffer that is full and holds no record (pair): a longer one
                    for s in ins:
                        if not s.eof and s.n_rec < grow_below:
                            s.grow()
                    continue
                done = all_eof or pending is not None
                if n:
                    client.check(ins, n)
                if pending is not None:
                    raise ValueError(pending)
                if n == 0:
                    break
                for s, used in zip(ins, client.emit(ins, n, files, writer)):
                    s.consume(used, n)
            result = client.result()
        for f in files:
            f.close()
        for tmp, o in zip(tmps, outs):
            os.replace(tmp, o)
    finally:
        for s in ins:
            s.close()
        for f in files:
            f.close()
        for tmp in tmps:
            if os.path.exists(tmp):
                os.remove(tmp)
    return result
