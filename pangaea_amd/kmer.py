"""Device tables of global canonical k-mer multiplicities and the per-run feature rows.

Mirrors, in one process and on the GPU, what ``src/feature.py`` obtains from three subprocesses:
``jellyfish count/dump`` (feature.py:94,103) -> :class:`KmerTable`; ``count_tnf`` (feature.py:133) and
``count_kmer`` (feature.py:109) -> :func:`features`.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib, fastqtext, readops
from .fastqtext import stream_ptr as _stream_ptr
from .reads import ReadStream, Rows

DEFAULT_SEG_CHARS = 65536              # row segments of the lookup kernels (K1: every segment ends in 136 global adds; 16384: 0.98 ms, 65536: 0.83 ms at 10 M pairs)


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} must live on a GPU: the k-mer kernels have no CPU path "
                           f"(got a tensor on {t.device})")


def _merged_lookups() -> bool:
    """the merged form of the super-k-mer lookups (provisional words in fixed slots per record); PG_MINI_MERGE=0: word-wise"""
    return os.environ.get("PG_MINI_MERGE", "1") not in ("", "0")


def mini_find_wanted() -> bool:
    """abundance rows against a finished mini table in super-k-mer form (``KmerTable.abundance_of``); PG_MINI_FIND=0, read at call
    time: the lookup form everywhere, as before that form existed"""
    return os.environ.get("PG_MINI_FIND", "1") not in ("", "0")


def _slack(n: int) -> int:
    """3 % of slack on a plan's counts: the next batch of the same size then finds room without asking"""
    return n + n // 32 + 4096


def _plan_head(ws: torch.Tensor) -> tuple:
    """(records, records of more than four k-mers) from the head of a plan workspace: 1st and 3rd word.  A host wait."""
    head = ws[:24].view(torch.int64).cpu()
    return int(head[0]), int(head[2])


# library calls that have a twin for a masked count half: the same arguments, the table plane's pointer behind the union plane's
_MASKED_TWIN = {"pg_mini_plan": "pg_mini_plan_masked", "pg_mini_count_half": "pg_mini_count_half_masked",
                "pg_mini_count_half_piece": "pg_mini_count_half_piece_masked"}


def _plain_or_masked(name: str, stream: ReadStream, plane: torch.Tensor, tab_plane: "torch.Tensor | None", *rest) -> None:
    """``name(codes, plane, *rest)`` or, where the table has a plane of its own (``tab_plane``: a masked count half, ``plane`` then
    being the union plane the kernels segment), its masked twin"""
    L = _lib.load()
    if tab_plane is None:
        _lib.check(getattr(L, name)(stream.codes.data_ptr(), plane.data_ptr(), *rest))
    else:
        _lib.check(getattr(L, _MASKED_TWIN[name])(stream.codes.data_ptr(), plane.data_ptr(), tab_plane.data_ptr(), *rest))


# what a mini table keeps between calls.  Named tuples on purpose: callers read them by position too.
# the plan in use: ``KmerTable._plan_key`` (("pieces", n) stands in after a count in pieces), the plan workspace, its record count,
# the rows, the tensors the key names (kept with the plan: see ``_plan_key``), its records of more than four k-mers.  The two
# counts are None while they are still on the device (``KmerTable.plan_counts`` reads them)
_MiniPlan = namedtuple("_MiniPlan", "key ws n_records rows held n_long")
_MiniNext = namedtuple("_MiniNext", "key ws event rows held")                  # a plan computed ahead on a side stream
_Half = namedtuple("_Half", "fill n_words rows window vsize")                  # between count_half and lookup_half
# a word range of a count in pieces: its plan, its 2-byte provisional slots, its bucket-ordered records' meta words, its words
_Piece = namedtuple("_Piece", "plan_ws merge_ws meta n_words")
# the arguments of a count to do again -- every one of them: ``lowercase_is_base`` decides the planes, ``world`` (a count half) the pieces
_Optimistic = namedtuple("_Optimistic", "stream word_begin word_end rows emit half lowercase_is_base world")


class KmerTable:
    """exact multiplicity of every canonical k-mer over every read of the input.

    ``dense``: int32 tensor of 4^k counters (k <= 16).  ``hash``: int64 tensor of 2^log2_slots slots,
    slot = (key42(code) << 22) | count, 0 = empty (k <= 21), optionally split into buckets of 2^log2_bucket slots
    (probing wraps inside a bucket); bucketed tables are built by the partition + LDS-count pipeline
    (``pg_kmer_count_bucketed``), unbucketed ones by one global atomic per occurrence (``pg_kmer_count``).
    ``wide`` (22 <= k <= 31, the rest of the reference's range): 2^log2_slots int64 keys (code + 1) followed by as
    many int32 counts in the same tensor; direct kernels only.
    """

    # bytes of scratch one bucketed launch may use (longer streams are counted in pieces): two 8-byte record buffers now, the
    # row shuffle adds half as much again later -- 132 GiB + 66 GiB + table + stream stay inside 288 GB of HBM and cover the
    # 25 M-pair share of BASELINE config 3 in one piece
    WORKSPACE_BUDGET = 132 << 30

    def __init__(self, k: int, kind: str, data: torch.Tensor, log2_slots: int = 0, log2_bucket: int = 0):
        self.k, self.kind, self.data, self.log2_slots, self.log2_bucket = int(k), kind, data, int(log2_slots), int(log2_bucket)
        self.status = torch.zeros(2, dtype=torch.int32, device=data.device)
        code = {"dense": _lib.TABLE_DENSE, "hash": _lib.TABLE_HASH, "wide": _lib.TABLE_WIDE, "mini": _lib.TABLE_MINI,
                "miniw": _lib.TABLE_MINI_WIDE}[kind]
        self._desc = _lib.pg_table(code, self.k, self.log2_slots, self.log2_bucket, data.data_ptr())
        self._empty = True               # nothing counted since allocation / reset()
        self._workspace = None
        self._shuffle_ws = None
        self._records = None             # (plan, n_words) while the workspace holds the row-tagged records of ONE count
        self._deferred = None            # (fill, n_words) after a deferred count: entries wait in the workspace, slots unwritten
        self._emitted = None             # (window, vsize) while the shuffle workspace holds the words of a fused count + lookup
        self._mini_plan = None           # _MiniPlan of the last pg_mini_plan: reused while the key matches
        self._mini_next = None           # _MiniNext: a plan computed ahead on a side stream
        self._mini_spare = None          # the plan workspace that is neither in use nor being filled
        self._mini_rec_ws = None
        self._mini_sized_for = None      # (n_words, geometry) the record / slot workspaces were sized for (with slack)
        self._mini_optimistic = None     # _Optimistic: the arguments of a count that ran on them without reading its plan's counts
        self.recounts = 0                # counts ``check_status`` did again because the kernels refused the kept workspaces (see ``count``)
        self._mini_pieces = 1            # word ranges the last count of a mini table was done in (``_count_mini_pieces``)
        self._half = None                # _Half, between count_half and lookup_half (N > 1 ranks)
        self._half_ws = None
        self._half_pieces = None         # ([_Piece], held tensors) of a count half in pieces
        self._half_world = 1             # ranks the count half's exchange goes to (its buffers count in the pieces decision)
        self._merge_ws = None            # the provisional words of the merged lookups (fixed slots per record)
        self.merge_form = None           # "aligned" / "general": which kernel built a table that ``merged`` returned
        self.combine_form = None         # "aligned" / "general": which kernel built a table that ``combined`` / ``filtered`` returned
        self.rows_form = None            # "find" / "lookup": how the last ``abundance_of`` built its rows
        self._depth_ws = None            # the workspace of ``depth``: the counts of its long ranges

    # ------------------------------------------------------------------ construction

    @staticmethod
    def default_kind(k: int) -> str:
        if k < 1 or k > _lib.WIDE_MAX_K:
            raise ValueError(f"k-mer size {k} unsupported (1..{_lib.WIDE_MAX_K}, as the reference)")
        if k > _lib.HASH_MAX_K:
            return "wide"
        # measured at 10 M pairs: k=15 dense 191 ms vs hash (partition + LDS) 70 ms; k=11 135 vs 69 ms.  Dense tables only
        # where 4^k counters stay cache resident.
        return "dense" if k <= 8 else "hash"

    @staticmethod
    def default_log2_bucket(log2_slots: int) -> int:
        """bucket size for a table of 2^log2_slots slots, 0 when the table cannot be bucketed: buckets hold at most
        2^14 slots (LDS) and there are at most 2^15 of them (two scatter passes)"""
        if log2_slots < 14:
            return 0                                       # small tables: the direct kernel is as good
        lb = min(_lib.BUCKET_MAX_LOG2_SLOTS, max(10, log2_slots - 12))
        return lb if 1 <= log2_slots - lb <= _lib.BUCKET_MAX_LOG2_BUCKETS else 0

    @classmethod
    def alloc(cls, k: int, device, kind: str | None = None, distinct_hint: int | None = None,
              load: float = 0.5, log2_bucket: int | None = None) -> "KmerTable":
        kind = kind or cls.default_kind(k)
        device = torch.device(device)
        if kind == "dense":
            if k > _lib.DENSE_MAX_K:
                raise ValueError(f"dense tables need k <= {_lib.DENSE_MAX_K}")
            return cls(k, "dense", torch.zeros(4 ** k, dtype=torch.int32, device=device))
        if kind in ("mini", "miniw"):
            want = max(1024, int((distinct_hint or 1 << 20) / load))
            return cls.mini_with_slots(k, device, max(10, math.ceil(math.log2(want))), log2_bucket)
        if kind not in ("hash", "wide"):
            raise ValueError(f"unknown table kind {kind!r}")
        if kind == "hash" and k > _lib.HASH_MAX_K:
            raise ValueError(f"hash tables need k <= {_lib.HASH_MAX_K}")
        want = max(1024, int((distinct_hint or 1 << 20) / load))
        log2 = max(10, math.ceil(math.log2(want)))
        if kind == "wide":
            return cls.wide_with_slots(k, device, log2)
        return cls.with_slots(k, device, log2, log2_bucket)

    @staticmethod
    def mini_max_log2_bucket(k: int) -> int:
        """slots of one LDS-resident bucket: 8-byte packed slots up to k = 21, 8-byte keys + 4-byte counts beyond"""
        return _lib.BUCKET_MAX_LOG2_SLOTS if k <= _lib.HASH_MAX_K else _lib.MINI_WIDE_MAX_LOG2_BUCKET_SLOTS

    @staticmethod
    def mini_default_log2_bucket(k: int, log2_slots: int) -> int:
        """bucket size of a mini table whose caller names none: the largest that LDS holds, except for packed tables (k <= 21) of
        2^(16 + 13) slots and more, which take buckets of 2^13 slots (two counting workgroups per CU), as many as the bucket count
        allows (PG_MINI_LARGE_LOG2_BUCKET_SLOTS)"""
        top = KmerTable.mini_max_log2_bucket(k)
        if k <= _lib.HASH_MAX_K and log2_slots >= _lib.MINI_MAX_LOG2_BUCKETS + _lib.MINI_LARGE_LOG2_BUCKET_SLOTS:
            return min(top, max(_lib.MINI_LARGE_LOG2_BUCKET_SLOTS, log2_slots - _lib.MINI_MAX_LOG2_BUCKETS))
        return min(top, log2_slots)

    @staticmethod
    def mini_applies(k: int, log2_slots: int, log2_bucket: int | None = None) -> bool:
        """can a MINI table (minimizer buckets, built from super-k-mers) hold 2^log2_slots slots for this k?"""
        if not _lib.MINI_MIN_K <= k <= _lib.WIDE_MAX_K:
            return False
        top = KmerTable.mini_max_log2_bucket(k)
        lb = min(top, log2_slots) if log2_bucket is None else log2_bucket
        return 4 <= lb <= top and 0 <= log2_slots - lb <= _lib.MINI_MAX_LOG2_BUCKETS

    @classmethod
    def mini_with_slots(cls, k: int, device, log2_slots: int, log2_bucket: int | None = None) -> "KmerTable":
        """``mini`` (k <= 21: packed 8-byte slots) or ``miniw`` (22 <= k <= 31: keys + counts planes, as ``wide``)"""
        top = cls.mini_max_log2_bucket(k)
        lb = cls.mini_default_log2_bucket(k, log2_slots) if log2_bucket is None else log2_bucket
        want = os.environ.get("PG_MINI_LOG2_BUCKET")            # tuning / comparison: bucket size of tables whose caller named none
        if log2_bucket is None and want and cls.mini_applies(k, log2_slots, min(int(want), top, log2_slots)):
            lb = min(int(want), top, log2_slots)
        if not cls.mini_applies(k, log2_slots, lb):
            raise ValueError(f"mini tables need {_lib.MINI_MIN_K} <= k <= {_lib.WIDE_MAX_K} and at most 2^{_lib.MINI_MAX_LOG2_BUCKETS} buckets "
                             f"of at most 2^{top} slots (k {k}, 2^{log2_slots} slots, buckets of 2^{lb})")
        n = 1 << log2_slots
        if k > _lib.HASH_MAX_K:
            return cls(k, "miniw", torch.zeros(n + n // 2, dtype=torch.int64, device=device), log2_slots, lb)
        return cls(k, "mini", torch.zeros(n, dtype=torch.int64, device=device), log2_slots, lb)

    @classmethod
    def wide_with_slots(cls, k: int, device, log2_slots: int) -> "KmerTable":
        n = 1 << log2_slots
        return cls(k, "wide", torch.zeros(n + n // 2, dtype=torch.int64, device=device), log2_slots, 0)

    def _wide_parts(self):
        n = 1 << self.log2_slots
        return self.data[:n], self.data[n:].view(torch.int32)

    @classmethod
    def with_slots(cls, k: int, device, log2_slots: int, log2_bucket: int | None = None) -> "KmerTable":
        lb = cls.default_log2_bucket(log2_slots) if log2_bucket is None else log2_bucket
        return cls(k, "hash", torch.zeros(1 << log2_slots, dtype=torch.int64, device=device), log2_slots, lb)

    @classmethod
    def from_items(cls, k: int, codes, counts, device, kind: str | None = None, distinct_hint: int | None = None) -> "KmerTable":
        """table holding exactly the given (canonical code, count) entries -- e.g. a parsed jellyfish dump
        (count_kmer.cpp:139-170 assigns, it does not add: later duplicates must already be resolved).  ``codes`` a tensor on a
        GPU (then ``counts`` too; int64 or uint64): the entries stay on the device -- what ``from_dump`` hands over -- and the
        table is the one the same entries make as numpy arrays.  ``distinct_hint``: size the table for that many entries
        rather than for the number given (a caller that grows the table after PG_ETABLEFULL)."""
        on_device = isinstance(codes, torch.Tensor) and codes.is_cuda
        if on_device:
            if not (isinstance(counts, torch.Tensor) and counts.is_cuda) or codes.numel() != counts.numel():
                raise ValueError("codes on the device need as many counts on the device")
            codes, counts = codes.reshape(-1).view(torch.int64), counts.reshape(-1).view(torch.int64)
        else:
            codes = torch.as_tensor(np.asarray(codes).astype(np.int64))
            counts = torch.as_tensor(np.asarray(counts).astype(np.int64))
        table = cls.alloc(k, device, kind, distinct_hint=max(1024, codes.numel(), distinct_hint or 0))
        if table.kind in ("wide", "miniw"):
            c = codes.to(table.device).contiguous()
            n = counts.to(table.device, torch.int32).contiguous()
            table._empty = False
            with torch.cuda.device(table.device):
                _lib.check(_lib.load().pg_kmer_merge_wide(c.data_ptr(), n.data_ptr(), c.numel(), table.desc(), table.status.data_ptr(),
                                                          _stream_ptr(table.device)))
            table.check_status()
        elif table.kind == "dense":
            table.data[codes.to(table.device)] = counts.to(table.device, torch.int32)
        elif table.kind == "mini":                     # the slots hold the codes themselves
            sat = torch.clamp(counts, max=_lib.HASH_COUNT_SAT)
            table.merge(((codes << _lib.HASH_COUNT_BITS) | sat)[sat > 0])
        else:
            sat = torch.clamp(counts, max=_lib.HASH_COUNT_SAT)
            keys = key42_torch(codes) if on_device else torch.from_numpy(key42(codes.numpy().view(np.uint64)).view(np.int64))
            table.merge(((keys << _lib.HASH_COUNT_BITS) | sat)[sat > 0])
        return table

    # ------------------------------------------------------------------ jellyfish's text dump (feature.py:87,103; count_kmer.cpp:139-170)

    DUMP_PIECE_BYTES = 256 << 20           # text per piece of ``write_dump`` / ``from_dump`` (device buffer + pinned host buffer)

    @staticmethod
    def _dump_piece_bytes() -> int:
        """PG_DUMP_PIECE_BYTES overrides the piece size (tests: pieces that start mid-table, lines across every boundary)"""
        want = os.environ.get("PG_DUMP_PIECE_BYTES")
        return max(256, int(want)) if want else KmerTable.DUMP_PIECE_BYTES

    @property
    def n_entries(self) -> int:
        return 4 ** self.k if self.kind == "dense" else 1 << self.log2_slots

    def write_dump(self, path: str, lower: int = 1) -> tuple:
        """the table as ``jellyfish dump -c -t -L lower`` writes it (the abundance.k{k}.dump of src/feature.py:87,103): one line
        ``<k-mer>\t<count>\n`` per entry with count >= ``lower``, in slot order -- for a given table always the same bytes.  A
        packed table (k <= 21, not dense) writes HASH_COUNT_SAT for every count at or above it.  Formatted on the device unit
        range by unit range, each piece at most ``DUMP_PIECE_BYTES`` of text, copied to pinned memory and appended; the file
        appears under its name only when it is complete.  Returns (lines, bytes)."""
        lower = int(lower)
        if lower < 1:
            raise ValueError(f"lower must be at least 1 (got {lower})")
        self._require_readable()
        L = _lib.load()
        n_units = (self.n_entries + _lib.DUMP_UNIT_SLOTS - 1) // _lib.DUMP_UNIT_SLOTS
        dev = self.device
        tmp = path + ".tmp"
        try:
            with torch.cuda.device(dev), open(tmp, "wb") as f:
                sizes = torch.empty((2, n_units), dtype=torch.int64, device=dev)
                _lib.check(L.pg_table_dump_sizes(self.desc(), lower, sizes[0].data_ptr(), sizes[1].data_ptr(), _stream_ptr(dev)))
                offsets = torch.zeros(n_units + 1, dtype=torch.int64, device=dev)
                torch.cumsum(sizes[0], 0, out=offsets[1:])
                lines = int(sizes[1].sum().item())
                off = offsets.cpu().numpy()
                total = int(off[-1])
                # unit ranges of at most a piece of text (a single unit may be more than a small piece: it then is a piece)
                piece = self._dump_piece_bytes()
                ranges, u0 = [], 0
                while u0 < n_units:
                    u1 = max(u0 + 1, int(np.searchsorted(off, off[u0] + piece, side="right")) - 1)
                    ranges.append((u0, u1))
                    u0 = u1
                room = max((int(off[b] - off[a]) for a, b in ranges), default=0)
                if room:
                    text = torch.empty(room, dtype=torch.uint8, device=dev)
                    host = torch.empty(room, dtype=torch.uint8, pin_memory=True)
                for a, b in ranges:
                    nb = int(off[b] - off[a])
                    if nb == 0:
                        continue
                    _lib.check(L.pg_table_dump_text(self.desc(), lower, a, b, offsets.data_ptr(), int(off[a]), nb, text.data_ptr(), room,
                                                    _stream_ptr(dev)))
                    host[:nb].copy_(text[:nb], non_blocking=True)
                    torch.cuda.current_stream(dev).synchronize()
                    f.write(memoryview(host.numpy())[:nb])
            os.replace(tmp, path)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return lines, total

    @classmethod
    def from_dump(cls, path: str, k: int, device, kind: str | None = None) -> "KmerTable":
        """table of a jellyfish text dump (``dump -c -t``; plain text, as the reference reads it), with the loader semantics of
        count_kmer.cpp:139-170 as ``cli.load_dump`` states them: later lines override earlier ones, k-mers with a character
        outside ACGT are dropped, blank lines skipped, CRLF tolerated; a k-mer of another length than ``k`` or a malformed count
        raises ValueError with the line.  The file is read piece by piece (cut behind the last newline, the rest carried into the
        next piece) into pinned memory, parsed on the device, and the entries never come back to the host."""
        k = int(k)
        if not 1 <= k <= _lib.WIDE_MAX_K:
            raise ValueError(f"k-mer size {k} unsupported (1..{_lib.WIDE_MAX_K}, as the reference)")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"the dump is parsed on a GPU: there is no CPU path (got {device})")
        L = _lib.load()
        piece = cls._dump_piece_bytes()
        codes, counts, ordinals = [], [], []
        with torch.cuda.device(device), open(path, "rb", buffering=0) as f:
            sp = _stream_ptr(device)
            host = torch.empty(piece, dtype=torch.uint8, pin_memory=True)
            buf = host.numpy()
            text = torch.empty(piece + 16, dtype=torch.uint8, device=device)
            cap = piece // (k + 2) + 1                                    # a kept line has k + 2 bytes at least
            out = torch.empty((3, cap), dtype=torch.int64, device=device)
            ws = torch.empty(_lib.check(L.pg_dump_parse_workspace_bytes(piece)), dtype=torch.uint8, device=device)
            word = torch.empty(3, dtype=torch.int64, device=device)       # kept lines, lines, status
            have, line0, eof = 0, 0, False
            while not eof:
                end = have
                while end < piece:
                    got = f.readinto(memoryview(buf)[end:])
                    if not got:
                        break
                    end += got
                eof = end < piece
                cut = end
                if not eof:
                    # behind the last newline; a piece without any holds a line no dump has (the parser says which)
                    at = end
                    while at > 0:
                        lo = max(0, at - 4096)
                        j = buf[lo:at].tobytes().rfind(b"\n")
                        if j >= 0:
                            cut = lo + j + 1
                            break
                        at = lo
                if cut:
                    text[:cut].copy_(host[:cut], non_blocking=True)
                    _lib.check(L.pg_dump_parse(text.data_ptr(), cut, k, line0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), cap,
                                               word.data_ptr(), word[2:].data_ptr(), ws.data_ptr(), ws.numel(), sp))
                    n_kept, n_lines, status = (int(v) for v in word.cpu())   # (waits for the copy and the parse: ``host`` is free again)
                    if status != -1:
                        raise ValueError(_dump_error(path, k, status & ((1 << 64) - 1)))
                    if n_kept:
                        codes.append(out[0, :n_kept].clone())
                        counts.append(out[1, :n_kept].clone())
                        ordinals.append(out[2, :n_kept].clone())
                    line0 += n_lines
                have = end - cut
                if have:
                    buf[:have] = buf[cut:end].copy()
            del text, out, ws
            if not codes:
                empty = torch.zeros(0, dtype=torch.int64, device=device)
                return cls.from_items(k, empty, empty, device, kind)
            codes, counts, ordinals = torch.cat(codes), torch.cat(counts), torch.cat(ordinals)
            # later lines override earlier ones (count_kmer.cpp:166): file order, then a stable sort by code, the last of a run stays
            order = torch.argsort(ordinals)
            del ordinals
            sc, idx = torch.sort(codes[order], stable=True)
            last = torch.ones(sc.numel(), dtype=torch.bool, device=device)
            last[:-1] = sc[1:] != sc[:-1]
            return cls.from_items(k, sc[last], counts[order[idx[last]]], device, kind)

    @property
    def device(self) -> torch.device:
        return self.data.device

    @property
    def nbytes(self) -> int:
        return self.data.numel() * self.data.element_size()

    def desc(self):
        return C.byref(self._desc)

    # ------------------------------------------------------------------ counting

    def reset(self) -> "KmerTable":
        """forget every count.  Bucketed tables are not even cleared: the next count overwrites every slice."""
        if not (self.kind in ("hash", "mini", "miniw") and self.log2_bucket):
            self.data.zero_()
        self.status.zero_()
        self._empty = True
        self._records = None
        self._deferred = None
        self._emitted = None
        return self

    def _grown(self, name: str, need: int, dtype=torch.uint8, exact: bool = False, shrink: bool = False) -> torch.Tensor:
        """the workspace held in attribute ``name``, with room for ``need`` elements.  One that is too small is dropped BEFORE its
        successor is allocated (at 100 GB both would not fit) -- which is why this takes the attribute, not the tensor: a
        caller's reference would keep the old one alive.  ``exact``: any other size is replaced (a size that depends on the
        geometry alone); ``shrink``: so is one more than twice too large."""
        buf = getattr(self, name)
        n = -1 if buf is None else buf.numel()
        del buf
        if n < need or (exact and n != need) or (shrink and n > 2 * need):
            setattr(self, name, None)
            setattr(self, name, torch.empty(need, dtype=dtype, device=self.device))
        return getattr(self, name)

    def _workspace_for(self, n_words: int) -> torch.Tensor:
        return self._grown("_workspace", _lib.check(_lib.load().pg_kmer_count_workspace_bytes(n_words, self.desc())))

    def can_defer(self, n_words: int) -> bool:
        """may ``count(..., deferred_group=g)`` be used for a fresh count of ``n_words`` words?"""
        step = int(self.WORKSPACE_BUDGET // (2 * 8 * 32))
        return self._bucketed() and self._empty and self.log2_slots - self.log2_bucket > 8 and n_words <= step

    def _shuffle_workspace_for(self, n_words: int, n_rows: int, vsize: int) -> torch.Tensor:
        return self._grown("_shuffle_ws", _lib.check(_lib.load().pg_abundance_workspace_bytes(n_words, n_rows, vsize, self.desc())))

    def count(self, stream: ReadStream, word_begin: int = 0, word_end: int | None = None, check: bool = True,
              rows: "Plan | None" = None, deferred_group: int | None = None, emit: tuple | None = None,
              lowercase_is_base: bool = False) -> "KmerTable":
        """add the k-mers ending in words [word_begin, word_end) of the stream (asynchronous unless ``check``).
        With ``rows`` (a Plan of this stream's rows) a bucketed table also keeps the row-tagged partition records, which
        lets ``features`` build the abundance rows by shuffle instead of by table lookups.

        ``deferred_group`` = g (multi-GPU, ``can_defer``): this table has the geometry of the union over all ranks and
        is NOT written; 2^g adjacent buckets are counted together in LDS and only their occupied entries and the
        per-bucket fills are kept, for ``dist.exchange_table`` to gather and to rebuild the table from.  Until then the
        table holds no counts (``pending``).

        ``emit`` = (window, vector_size) (one GPU, a fresh table, ``rows`` given, at least 2^11 buckets): the lookup pass of
        the abundance rows is fused into the counting kernel -- a bucket's records are looked up while its counts are
        still in LDS -- and ``features`` with the same window and vector size starts from the emitted (row, bin) words.
        Silently ignored where it does not apply.

        ``lowercase_is_base``: count lower-case a c g t as bases, as ``jellyfish count`` does (src/feature.py:94) -- the
        reference's own row counters reset on them (count_kmer.cpp:73-78), so k-mers that are only valid under this rule
        enter the table but belong to no row.  Only matters for soft-masked input (``stream.valid_lower`` is not None).
        Paired input with bases below the quality threshold (``stream.valid_lowq``, jellyfish's --min-qual-char=? of
        feature.py:76-83) is always counted without them, and without ``rows`` / ``emit`` (see ``ReadStream.table_valid``).

        ``check=False`` on a mini table, the contract: a count that picked up a plan computed ahead (``prefetch_plan``) may run on
        the workspaces the previous batch sized without having read its plan's record counts.  If they turn out too small the
        kernels count NOTHING, and ``check_status()`` counts again with workspaces of the right size and adds one to
        ``self.recounts``.  So whatever was derived from the table between this call and ``check_status()`` -- ``features`` rows,
        ``items()``, an encode of those rows -- is void if ``recounts`` moved across ``check_status()``, and must be derived
        again.  (``check=True`` calls ``check_status()`` itself: nothing can lie in between.)"""
        _require_gpu(stream.codes, "the read stream")
        if stream.device != self.device:
            raise ValueError("stream and table are on different devices")
        word_end = stream.n_words if word_end is None else word_end
        L = _lib.load()
        # the table is counted with jellyfish's view of the reads (lower-case bases count when asked for, bases below the
        # quality threshold of paired input never do); rows keep the reference's own rule, the strict plane
        table_plane = stream.table_valid(lowercase_is_base)
        lenient = table_plane is not stream.valid
        valid_ptr = table_plane.data_ptr()
        if not stream.rows_inside_table:
            # quality-masked bases: a row's k-mer may be missing from the table, which only the lookup form of ``features``
            # expresses (count_kmer.cpp:87) -- no row-tagged records, no fused lookups
            rows = emit = None

        if self.kind in ("mini", "miniw"):
            if deferred_group is not None:
                raise ValueError("mini tables have no deferred form")
            return self._count_mini(stream, word_begin, word_end, table_plane, rows, emit, lenient, check, lowercase_is_base=lowercase_is_base)
        if deferred_group is not None:
            if not self.can_defer(word_end - word_begin):
                raise ValueError("deferred counting needs a fresh bucketed table with more than 256 buckets and a single pass")
            g = max(0, min(int(deferred_group), _lib.DEFERRED_MAX_GROUP_LOG2, self.log2_slots - self.log2_bucket - 8))
            keep = rows if (rows is not None and rows.shuffle_ok) else None
            ws = self._workspace_for(word_end - word_begin)
            fill = torch.empty(self.n_buckets, dtype=torch.int64, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(L.pg_kmer_count_deferred(stream.codes.data_ptr(), valid_ptr, word_begin, word_end, self.desc(), g,
                                                    self._rows_ref(keep, stream, lenient), ws.data_ptr(), ws.numel(),
                                                    fill.data_ptr(), self.status.data_ptr(), _stream_ptr(self.device)))
            self._empty = False
            self._deferred = (fill, word_end - word_begin)
            self._records = (keep, word_end - word_begin) if keep is not None else None
            if check:
                self.check_status()
            return self
        self._deferred = None
        self._emitted = None
        with torch.cuda.device(self.device):
            if self.kind == "hash" and self.log2_bucket:
                # pieces bounded by the scratch budget: two record buffers of 8 B per character
                step = max(_lib.WORD_ALIGN, int(self.WORKSPACE_BUDGET // (2 * 8 * 32)) // _lib.WORD_ALIGN * _lib.WORD_ALIGN)
                single = self._empty and word_end - word_begin <= step
                keep = rows if (single and rows is not None and rows.shuffle_ok) else None
                self._records = None
                if (emit is not None and keep is not None and self._bucketed() and self.tag_bits <= 31 and word_end > word_begin
                        and 1 <= emit[1] <= _lib.SHUFFLE_MAX_VSIZE and emit[0] >= 1 and emit[0] * emit[1] <= _lib.HASH_COUNT_SAT):
                    window, vsize = int(emit[0]), int(emit[1])
                    n_words = word_end - word_begin
                    ws = self._workspace_for(n_words)
                    sws = self._shuffle_workspace_for(n_words, keep.n_rows, vsize)
                    _lib.check(L.pg_kmer_count_bucketed_emit(stream.codes.data_ptr(), valid_ptr, word_begin, word_end, self.desc(),
                                                             self._rows_ref(keep, stream, lenient), ws.data_ptr(), ws.numel(), window, vsize,
                                                             sws.data_ptr(), sws.numel(), self.status.data_ptr(), _stream_ptr(self.device)))
                    self._empty = False
                    self._records = (keep, n_words)
                    self._emitted = (window, vsize)
                    if check:
                        self.check_status()
                    return self
                for w0 in range(word_begin, word_end, step):
                    w1 = min(word_end, w0 + step)
                    ws = self._workspace_for(w1 - w0)
                    _lib.check(L.pg_kmer_count_bucketed(stream.codes.data_ptr(), valid_ptr, w0, w1, self.desc(),
                                                        0 if self._empty else 1, self._rows_ref(keep, stream, lenient),
                                                        ws.data_ptr(), ws.numel(), self.status.data_ptr(), _stream_ptr(self.device)))
                    self._empty = False
                if keep is not None:
                    self._records = (keep, word_end - word_begin)
            else:
                _lib.check(L.pg_kmer_count(stream.codes.data_ptr(), valid_ptr, word_begin, word_end,
                                           self.desc(), self.status.data_ptr(), _stream_ptr(self.device)))
                self._empty = False
        if check:
            self.check_status()
        return self

    @staticmethod
    def _plan_key(codes: torch.Tensor, plane: torch.Tensor, word_begin: int, word_end: int, keep, lenient: bool, log2_slots: int, log2_bucket: int):
        """what a cached partition plan is valid for.  Addresses alone would not do: after the stream is freed the caching
        allocator hands the same address to the next stream of that size, and tensors can be rewritten in place -- so the key
        carries the tensors' version counters, and the cache entry holds the tensors (and the rows) themselves, which keeps
        their storage from being recycled while the plan is kept.  (pg_mini_count checks the plan's record count against the
        record workspace as well: PG_STATUS_PLAN_MISMATCH.)"""
        return (codes.data_ptr(), codes._version, plane.data_ptr(), plane._version, word_begin, word_end, id(keep), bool(lenient),
                log2_slots, log2_bucket)

    @staticmethod
    def half_masked(stream: ReadStream, lowercase_is_base: bool = False) -> bool:
        """does ``count_half`` of this stream take the masked form (a table plane other than the rows' strict one)?"""
        return stream.table_valid(lowercase_is_base) is not stream.valid or not stream.rows_inside_table

    def count_half(self, stream: ReadStream, rows: "Plan", emit: tuple, check: bool = True, world: int = 1,
                   lowercase_is_base: bool = False) -> "KmerTable":
        """N > 1 ranks (``dist.MiniSharded``): the COUNT half of the super-k-mer pipeline on this rank's reads.  This table object
        only carries the rank's LOCAL geometry (the union's bucket count, slots for the rank's own k-mers): its slots are never
        written -- except by a count in pieces (``_count_half_pieces``; ``world`` sizes the exchange's buffers in that decision).
        Left behind for ``dist``: the buckets' entries and occupancy (``_half``), the provisional words of the rows.

        Masked input (``half_masked``: soft-masked reads with ``lowercase_is_base``, bases below the quality threshold): the
        table counts the k-mers of ``stream.table_valid(lowercase_is_base)``, the rows keep the strict plane ``stream.valid``, and
        the kernels segment their union (include/pangaea_feat.h: the masked count half).  A k-mer only a row sees takes a
        local slot with count 0 -- its entry asks the owners for the bin of whatever the other ranks counted (the owners must
        run ``pg_mini_merge_bins_masked``).  Needs the merged lookups and at most 2^19 - 2 rows."""
        if self.kind != "mini":
            raise ValueError("count_half() is for packed mini tables (13 <= k <= 21)")
        _require_gpu(stream.codes, "the read stream")
        self._half_world = int(world)
        if not self.half_masked(stream, lowercase_is_base):
            return self._count_mini(stream, 0, stream.n_words, stream.table_valid(False), rows, emit, False, check, half=True,
                                    lowercase_is_base=lowercase_is_base)
        if rows is None or rows.n_rows > _lib.MINI_MASKED_MAX_ROWS or not _merged_lookups():
            raise ValueError(f"count_half() of masked input needs the merged lookups and at most {_lib.MINI_MASKED_MAX_ROWS} rows")
        # (the rows' own rule: the strict plane rides along, as in ``count``)
        return self._count_mini(stream, 0, stream.n_words, stream.union_valid(lowercase_is_base), rows, emit, True, check,
                                half=True, tab_plane=stream.table_valid(lowercase_is_base), lowercase_is_base=lowercase_is_base)

    def _count_mini(self, stream, word_begin, word_end, table_plane, rows, emit, lenient, check, half=False, tab_plane=None,
                    lowercase_is_base=False):
        """the super-k-mer pipeline (pg_mini_plan + pg_mini_count): a fresh table, one piece.  The partition plan depends on
        the stream, the rows and the geometry only and is kept: counting the same range again skips pg_mini_plan.
        ``tab_plane`` (a masked count half): the table plane, ``table_plane`` then being the union plane the kernels segment."""
        if not self._empty:
            raise ValueError("mini tables are built by ONE count of a fresh (or reset) table")
        L = _lib.load()
        n_words = word_end - word_begin
        keep = rows if (rows is not None and rows.shuffle_ok and rows.n_rows <= _lib.MINI_MAX_ROWS) else None
        if rows is not None and keep is None:
            raise ValueError("mini tables need sorted, disjoint, non-empty rows (at most 2^20 - 2 of them)")
        fuse = (emit is not None and keep is not None and n_words > 0 and 1 <= emit[1] <= _lib.SHUFFLE_MAX_VSIZE and emit[0] >= 1
                and (self.kind == "miniw" or emit[0] * emit[1] <= _lib.HASH_COUNT_SAT))
        if half and not fuse:
            raise ValueError("count_half() needs rows and abundance parameters")
        window, vsize = (int(emit[0]), int(emit[1])) if fuse else (0, 0)
        rows_ref = self._rows_ref(keep, stream, lenient)
        # a stream whose scratch would not fit in one piece (about 3.4 KB per 150 bp read pair; PANGAEA_MINI_PIECE_WORDS forces a
        # piece size) is counted word range by word range into the same table, its lookups done when the table is final
        piece_words = self._piece_words(n_words, fuse and not half)
        if piece_words is not None:
            return self._count_mini_pieces(stream, word_begin, word_end, table_plane, keep, rows_ref, window, vsize, piece_words, check)
        self._half_pieces = None
        piece_words = self._half_piece_words(n_words, keep, vsize) if half else None
        if piece_words is not None:
            return self._count_half_pieces(stream, word_begin, word_end, table_plane, keep, rows_ref, window, vsize, piece_words, check, tab_plane)
        key = self._plan_key(stream.codes, table_plane, word_begin, word_end, keep, lenient, self.log2_slots, self.log2_bucket)
        held = (stream.codes, table_plane)               # (kept with the plan: see _plan_key)
        if tab_plane is not None:
            key += (tab_plane.data_ptr(), tab_plane._version, stream.valid.data_ptr(), stream.valid._version)
            held += (tab_plane, stream.valid)
        sp = _stream_ptr(self.device)
        with torch.cuda.device(self.device):
            if (self._mini_plan is None or self._mini_plan.key != key) and not self._take_prefetched_plan(key, n_words, keep, held):
                self._compute_plan(key, stream, table_plane, tab_plane, word_begin, word_end, keep, rows_ref, held)
            plan_ws, n_records, n_long = self._mini_plan.ws, self._mini_plan.n_records, self._mini_plan.n_long
            optimistic = n_records is None          # (workspaces of the previous batch of this size, the plan's counts unread)
            if not optimistic:
                # (``shrink``: a batch much smaller than the last gives the difference back)
                self._grown("_mini_rec_ws", _lib.check(L.pg_mini_records_bytes(_slack(n_records), self.desc())), shrink=True)
                self._mini_sized_for = (n_words, self.log2_slots, self.log2_bucket)
            sws_ptr, sws_n = None, 0
            if fuse:
                # (with the merged lookups the provisional data live in their own buffer below: the row shuffle's layout is smaller)
                sws = self._grown("_shuffle_ws", _lib.check(L.pg_mini_shuffle_bytes_merged(n_words, keep.n_rows, vsize, self.desc()) if _merged_lookups()
                                                            else L.pg_mini_shuffle_bytes(n_words, keep.n_rows, vsize)))
                sws_ptr, sws_n = sws.data_ptr(), sws.numel()
            mws_ptr, mws_n = None, 0
            if fuse and _merged_lookups():
                # the merged form of the lookups: its provisional words lie in fixed slots per record, sized from the plan's record
                # counts; the library falls back to the word-wise form where the merged one does not apply
                if not optimistic or self._merge_ws is None:
                    if optimistic:                                         # (no slot buffer yet: the counts are needed after all)
                        n_records, n_long = self.plan_counts()
                        optimistic = False
                    self._grown("_merge_ws", _lib.check(L.pg_mini_merge_words(n_words, _slack(n_records), min(_slack(n_long), _slack(n_records)), self.desc())),
                                dtype=torch.int32)
                mws_ptr, mws_n = self._merge_ws.data_ptr(), self._merge_ws.numel()
            rec_ws = self._mini_rec_ws
            args = (word_begin, word_end, self.desc(), rows_ref, plan_ws.data_ptr(), plan_ws.numel(), rec_ws.data_ptr(), rec_ws.numel(),
                    window, vsize, sws_ptr, sws_n, mws_ptr, mws_n)
            if half:
                half_ws, fill = self._half_workspaces()
                _plain_or_masked("pg_mini_count_half", stream, table_plane, tab_plane, *args, half_ws.data_ptr(), half_ws.numel(),
                                 fill.data_ptr(), self.status.data_ptr(), sp)
                self._half = _Half(fill, n_words, keep, window, vsize)
            else:
                _lib.check(L.pg_mini_count(stream.codes.data_ptr(), table_plane.data_ptr(), *args, self.status.data_ptr(), sp))
        self._empty = False
        self._mini_pieces = 1
        self._records = (keep, n_words) if fuse and not half else None
        self._emitted = (window, vsize) if fuse and not half else None
        self._mini_optimistic = (_Optimistic(stream, word_begin, word_end, rows, emit, half, bool(lowercase_is_base),
                                             self._half_world if half else 1)
                                 if optimistic else None)
        if check:
            self.check_status()
        return self

    def _take_prefetched_plan(self, key, n_words: int, keep, held) -> bool:
        """a plan computed ahead (``prefetch_plan``) for this key becomes the plan in use: the count waits for it ON THE DEVICE.
        Its record counts size the record and slot workspaces -- but where workspaces of a batch of the same size exist already (a
        stream of batches), they are used as they are and the host does not wait for the plan at all: the kernels themselves refuse
        a plan that names more records than the buffers hold (PG_STATUS_PLAN_MISMATCH, nothing is written), and ``check_status``
        then counts again with workspaces of the right size.  The counts stay on the device until somebody asks (``plan_counts``).
        False: no such plan."""
        ahead = self._mini_next
        if ahead is None or ahead.key != key:
            return False
        torch.cuda.current_stream(self.device).wait_event(ahead.event)
        if self._mini_plan is not None:
            self._mini_spare = self._mini_plan.ws
        if (self._mini_sized_for == (n_words, self.log2_slots, self.log2_bucket) and self._mini_rec_ws is not None
                and os.environ.get("PG_PLAN_HOST_SYNC", "0") in ("", "0")):
            self._mini_plan = _MiniPlan(key, ahead.ws, None, keep, held, None)
        else:
            ahead.event.synchronize()
            n_records, n_long = _plan_head(ahead.ws)
            self._mini_plan = _MiniPlan(key, ahead.ws, n_records, keep, held, n_long)
        self._mini_next = None
        return True

    def _compute_plan(self, key, stream, table_plane, tab_plane, word_begin, word_end, keep, rows_ref, held) -> None:
        """pg_mini_plan in front of its count, into the spare plan workspace where that has the size; one host wait for its counts"""
        need = _lib.check(_lib.load().pg_mini_plan_bytes(word_end - word_begin, self.desc()))
        ws = self._mini_spare if self._mini_spare is not None and self._mini_spare.numel() == need else None
        self._mini_spare = None
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        _plain_or_masked("pg_mini_plan", stream, table_plane, tab_plane, word_begin, word_end, self.desc(), rows_ref,
                         ws.data_ptr(), ws.numel(), _stream_ptr(self.device))
        n_records, n_long = _plan_head(ws)                             # (host sync; once per plan)
        if self._mini_plan is not None:
            self._mini_spare = self._mini_plan.ws
        self._mini_plan = _MiniPlan(key, ws, n_records, keep, held, n_long)

    def _rows_ref(self, plan, stream: ReadStream, lenient: bool):
        """the rows argument of a library call (None without rows).  The rows' own validity rule stays the strict one: where the
        table is counted under a lenient plane, the strict plane rides along."""
        if plan is None:
            return None
        if not lenient:
            return C.byref(plan.rows_desc)
        self._rows_desc_keepalive = _lib.pg_rows(plan.row_start.data_ptr(), plan.row_end.data_ptr(), plan.n_rows, stream.valid.data_ptr())
        return C.byref(self._rows_desc_keepalive)

    def _half_workspaces(self) -> tuple:
        """(entry slabs and occupancy of a count half, the buckets' fills).  The fills are zeroed: a count half that refuses its plan
        -- PG_STATUS_PLAN_MISMATCH -- writes nothing, and the exchange sizes its buffers from these numbers before anybody has
        looked at the status word."""
        # (``exact``: the size is a function of the geometry alone)
        half_ws = self._grown("_half_ws", _lib.check(_lib.load().pg_mini_half_bytes(self.desc())), exact=True)
        return half_ws, torch.zeros(self.n_buckets, dtype=torch.int64, device=self.device)

    # bytes of scratch per word of the stream (32 characters): record workspace (two planes of 12-byte records, ~6.7 records per
    # word at k = 21), 2-byte slots of the merged lookups, the row shuffle's word regions (4 bytes per character)
    _PIECE_BYTES_PER_WORD = (24 * 7, 12 * 7, 4 * 32)

    def _pieces_apply(self) -> bool:
        """the pieces' kernels: packed slots, both scatter passes, the merged lookups"""
        return self.kind == "mini" and self.n_buckets > 256 and _merged_lookups()

    @staticmethod
    def _forced_piece_words(n_words: int):
        """(forced, words per piece or None for one piece) of PANGAEA_MINI_PIECE_WORDS"""
        forced = os.environ.get("PANGAEA_MINI_PIECE_WORDS")
        if not forced:
            return False, None
        w = max(_lib.WORD_ALIGN, int(forced) // _lib.WORD_ALIGN * _lib.WORD_ALIGN)
        return True, (w if w < n_words else None)

    def _free_bytes(self) -> int:
        free, _ = torch.cuda.mem_get_info(self.device)
        return free + torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)      # (cached blocks count as free)

    def _piece_words(self, n_words: int, applicable: bool):
        """None (one piece, the usual path) or the number of words per piece"""
        if not applicable or not self._pieces_apply():
            return None
        forced, w = self._forced_piece_words(n_words)
        if forced:
            return w
        rec, slots, words = self._PIECE_BYTES_PER_WORD
        budget = 0.85 * self._free_bytes()
        if (rec + slots + words) * n_words <= budget:
            return None
        room = budget - (slots + words + 4 * 7) * n_words          # what stays per word whatever the piece size (slots, kept meta, words)
        if room <= rec * 4 * _lib.WORD_ALIGN:
            return None                                          # (not even in pieces: the one-piece path reports the allocation that fails)
        return max(_lib.WORD_ALIGN, int(room / rec) // _lib.WORD_ALIGN * _lib.WORD_ALIGN)

    def _half_piece_words(self, n_words: int, keep: "Plan", vsize: int):
        """``_piece_words`` for a count half (N > 1 ranks): None (one piece) or the words per piece.  PANGAEA_MINI_PIECE_WORDS forces
        a piece size as on one GPU; otherwise ``half_piece_words`` decides from the free device memory, to which the workspaces this
        table holds from an earlier count are added back (they are reused or replaced)."""
        if not self._pieces_apply() or _lib.check(_lib.load().pg_mini_merge_form_applies(self.desc(), keep.n_rows, vsize)) != 1:
            return None
        forced, w = self._forced_piece_words(n_words)
        if forced:
            return w
        held = [self._mini_rec_ws, self._shuffle_ws, self._merge_ws, self._half_ws] + ([self.data] if self.data.numel() > 1 else [])
        free = self._free_bytes() + sum(int(t.numel()) * t.element_size() for t in held if t is not None)
        w = half_piece_words(free, n_words, self.log2_slots, self.log2_bucket, keep.n_rows, self._half_world)
        return w if w is not None and w < n_words else None

    def _count_pieces(self, stream, word_begin, word_end, piece_words, table_plane, tab_plane, rows_ref, count) -> list:
        """the piece loop of a count in word ranges of ``piece_words``: every range -> its plan (a host wait for its counts), a
        record workspace that holds it (one for all pieces, grown where a piece needs more), the 2-byte provisional slots of its
        merged lookups, then ``count(w0, w1, first, last, plan_ws, rec_ws, merge_ws)`` -- the caller's library call -- and the
        records' meta words copied out.  Returns what the lookups need, a ``_Piece`` per range; the table is no longer empty.  (``count`` is a callback so that
        nobody but this loop holds the record workspace: it is dropped before a larger one is allocated, and on return.)"""
        L = _lib.load()
        sp = _stream_ptr(self.device)
        ranges = [(w0, min(word_end, w0 + piece_words)) for w0 in range(word_begin, word_end, piece_words)]
        kept, rec_ws = [], None
        for idx, (w0, w1) in enumerate(ranges):
            plan_ws = torch.empty(_lib.check(L.pg_mini_plan_bytes(w1 - w0, self.desc())), dtype=torch.uint8, device=self.device)
            _plain_or_masked("pg_mini_plan", stream, table_plane, tab_plane, w0, w1, self.desc(), rows_ref, plan_ws.data_ptr(), plan_ws.numel(), sp)
            n_records, n_long = _plan_head(plan_ws)                    # (host wait, once per piece)
            need = _lib.check(L.pg_mini_records_bytes(_slack(n_records), self.desc()))
            if rec_ws is None or rec_ws.numel() < need:
                rec_ws = None                                          # (dropped first, as ``_grown`` does)
                rec_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            merge_ws = torch.empty(_lib.check(L.pg_mini_merge_words(w1 - w0, n_records, n_long, self.desc())), dtype=torch.int32, device=self.device)
            count(w0, w1, 1 if idx == 0 else 0, 1 if idx == len(ranges) - 1 else 0, plan_ws, rec_ws, merge_ws)
            # the bucket-ordered records' meta words (lengths, rows): the second meta plane of [bases A | bases B | meta A | meta B]
            moff = _lib.check(L.pg_mini_records_meta_offset(rec_ws.numel(), self.desc()))
            kept.append(_Piece(plan_ws, merge_ws, rec_ws[moff: moff + 4 * n_records].view(torch.int32).clone(), w1 - w0))
        self._empty = False
        self._mini_pieces = len(kept)
        self._mini_optimistic = None
        return kept

    def _lookup_pieces(self, pieces, keep, held, n_words: int, window: int, vsize: int, rows_ref, lookup) -> None:
        """the lookups of a count in pieces, once the table is final: the row shuffle's regions of the whole stream prepared once
        (pg_mini_lookup_begin), then ``lookup(piece, sws)`` -- the caller's library call -- for every piece; ``features`` then reads
        the rows from the shuffled words as after one count"""
        L = _lib.load()
        with torch.cuda.device(self.device):
            sws = self._grown("_shuffle_ws", _lib.check(L.pg_mini_shuffle_bytes_merged(n_words, keep.n_rows, vsize, self.desc())))
            _lib.check(L.pg_mini_lookup_begin(self.desc(), rows_ref, n_words, vsize, sws.data_ptr(), sws.numel(), _stream_ptr(self.device)))
            for piece in pieces:
                lookup(piece, sws)
            # (``abundance_from_records`` hands a plan workspace of the whole range to pg_mini_abundance_from_emitted, which only checks its
            # size: a stand-in takes the place of the plan in use)
            whole = torch.empty(_lib.check(L.pg_mini_plan_bytes(n_words, self.desc())), dtype=torch.uint8, device=self.device)
        self._mini_plan = _MiniPlan(("pieces", len(pieces)), whole, sum(int(p.meta.numel()) for p in pieces), keep, held, 0)
        self._records = (keep, n_words)
        self._emitted = (window, vsize)

    def _count_mini_pieces(self, stream, word_begin, word_end, table_plane, keep, rows_ref, window, vsize, piece_words, check):
        """``_count_mini`` for a stream counted in word ranges of ``piece_words`` (include/pangaea_feat.h: pg_mini_count_piece):
        every piece -> its plan, both scatter passes, the count INTO the table's buckets (slots keep their places), its 2-byte
        provisional slots and its records' meta words kept; then the lookups of every piece in the final table, into the row
        shuffle's regions of the whole stream.  Afterwards the table is what one count would have made it (``features`` reads
        the rows from the shuffled words as usual)."""
        L = _lib.load()
        n_words = word_end - word_begin
        sp = _stream_ptr(self.device)

        def count(w0, w1, first, last, plan_ws, rec_ws, merge_ws):
            _lib.check(L.pg_mini_count_piece(stream.codes.data_ptr(), table_plane.data_ptr(), w0, w1, self.desc(), rows_ref, plan_ws.data_ptr(), plan_ws.numel(),
                                             rec_ws.data_ptr(), rec_ws.numel(), window, vsize, merge_ws.data_ptr(), merge_ws.numel(),
                                             first, self.status.data_ptr(), sp))

        def lookup(piece, sws):
            _lib.check(L.pg_mini_lookup_piece(self.desc(), rows_ref, piece.plan_ws.data_ptr(), piece.plan_ws.numel(), piece.n_words, piece.meta.data_ptr(),
                                              n_words, window, vsize, sws.data_ptr(), sws.numel(), piece.merge_ws.data_ptr(), self.status.data_ptr(), sp))

        with torch.cuda.device(self.device):
            kept = self._count_pieces(stream, word_begin, word_end, piece_words, table_plane, None, rows_ref, count)
        self._lookup_pieces(kept, keep, (stream.codes, table_plane), n_words, window, vsize, rows_ref, lookup)
        if check:
            self.check_status()
        return self

    def _count_half_pieces(self, stream, word_begin, word_end, table_plane, keep, rows_ref, window, vsize, piece_words, check, tab_plane=None):
        """the count half (``count_half``) of a stream counted in word ranges of ``piece_words`` (include/pangaea_feat.h:
        pg_mini_count_half_piece): every piece -> its plan, both scatter passes, the count INTO this table's own slots (allocated
        here: 8 bytes x 2^log2_slots), its 2-byte provisional slots and its records' meta words kept; the last piece leaves entries,
        occupancy and fill as one count half does.  ``lookup_half`` then looks every piece up with the bins the owners sent back."""
        sp = _stream_ptr(self.device)
        if self.data.numel() != 1 << self.log2_slots:            # (the slots the pieces count into: every slot is written by the first piece)
            self.data = torch.empty(1 << self.log2_slots, dtype=torch.int64, device=self.device)
            self._desc.data = self.data.data_ptr()
        # (the one-piece workspaces are not used on this path: their memory goes back to the allocator)
        self._mini_rec_ws = self._merge_ws = None
        self._mini_plan = None
        with torch.cuda.device(self.device):
            half_ws, fill = self._half_workspaces()

            def count(w0, w1, first, last, plan_ws, rec_ws, merge_ws):
                _plain_or_masked("pg_mini_count_half_piece", stream, table_plane, tab_plane, w0, w1, self.desc(), rows_ref,
                                 plan_ws.data_ptr(), plan_ws.numel(), rec_ws.data_ptr(), rec_ws.numel(), window, vsize,
                                 merge_ws.data_ptr(), merge_ws.numel(), half_ws.data_ptr(), half_ws.numel(),
                                 fill.data_ptr(), first, last, self.status.data_ptr(), sp)

            kept = self._count_pieces(stream, word_begin, word_end, piece_words, table_plane, tab_plane, rows_ref, count)
        self._half = _Half(fill, word_end - word_begin, keep, window, vsize)
        self._half_pieces = (kept, (stream.codes, table_plane) + (() if tab_plane is None else (tab_plane, stream.valid)))
        self._records = self._emitted = None
        if check:
            self.check_status()
        return self

    def plan_counts(self) -> tuple:
        """(records, records of more than four k-mers) of the partition plan in use -- read from the device on first use (a plan
        picked up without a host wait keeps them there)"""
        plan = self._mini_plan
        if plan.n_records is None:
            n_records, n_long = _plan_head(plan.ws)
            plan = self._mini_plan = plan._replace(n_records=n_records, n_long=n_long)
        return plan.n_records, plan.n_long

    def lookup_half(self, bins: torch.Tensor, bin_elem: torch.Tensor) -> None:
        """N > 1 ranks: finish a ``count_half`` -- ``bins`` (int16 view of what the bucket owners sent back: bin + 1 of every entry in
        the merged table, in the order the entries were sent), ``bin_elem[b]`` = where bucket b's bins start -- lookups of the
        provisional words and the row-group scatter; ``features`` then reads the rows from the shuffled words.

        After a count half in pieces every piece's provisional slots are looked up with the bins, and the pieces stay kept: an
        exchange done again (``MiniSharded.count`` after PG_STATUS_OVERFLOW_LIST) is looked up again without a recount."""
        half = self._half
        assert bins.dtype == torch.int16 and bin_elem.dtype == torch.int64 and bin_elem.numel() == self.n_buckets
        L = _lib.load()
        sp = _stream_ptr(self.device)
        rows_ref = C.byref(half.rows.rows_desc)
        half_ws = self._half_ws
        if self._half_pieces is not None:
            pieces, held = self._half_pieces

            def lookup(piece, sws):
                _lib.check(L.pg_mini_lookup_half_piece(self.desc(), rows_ref, piece.plan_ws.data_ptr(), piece.plan_ws.numel(), piece.n_words,
                                                       piece.meta.data_ptr(), half.n_words, half.vsize, sws.data_ptr(), sws.numel(),
                                                       piece.merge_ws.data_ptr(), half_ws.data_ptr(), half_ws.numel(), bins.data_ptr(),
                                                       bin_elem.data_ptr(), self.status.data_ptr(), sp))

            self._lookup_pieces(pieces, half.rows, held, half.n_words, half.window, half.vsize, rows_ref, lookup)
            return
        plan_ws = self._mini_plan.ws
        with torch.cuda.device(self.device):
            _lib.check(L.pg_mini_lookup_half(self.desc(), rows_ref, plan_ws.data_ptr(), plan_ws.numel(),
                                             self._mini_rec_ws.data_ptr(), self._mini_rec_ws.numel(), half.n_words, half.vsize,
                                             self._shuffle_ws.data_ptr(), self._shuffle_ws.numel(),
                                             self._merge_ws.data_ptr() if self._merge_ws is not None else None,
                                             self._merge_ws.numel() if self._merge_ws is not None else 0,
                                             half_ws.data_ptr(), half_ws.numel(),
                                             bins.data_ptr(), bin_elem.data_ptr(), self.status.data_ptr(), sp))
        self._records = (half.rows, half.n_words)
        self._emitted = (half.window, half.vsize)
        self._half = None

    def can_reexchange(self) -> bool:
        """does this table still hold what the exchange sends (a count half in pieces keeps its entries, fills and pieces until
        the next count)?"""
        return self._half is not None and self._half_pieces is not None

    def prefetch_plan(self, stream: ReadStream, rows: "Plan | None", side: "torch.cuda.Stream",
                      after: "torch.cuda.Event | None" = None) -> None:
        """compute the partition plan of the NEXT count of ``stream`` (whole range, strict validity) on the stream ``side``, into a
        workspace of its own: ``side`` waits for what the current stream has enqueued so far -- call this right after ``count`` and
        the plan of batch i + 1 runs under the row histograms and the encode of batch i instead of in front of its own count.
        The next ``count`` of the same stream and rows picks it up (and waits for it); any other count ignores it.

        Where workspaces of a batch of the same size exist, that count does not read the plan's record counts on the host: see
        ``count`` for what that means to a caller who passes ``check=False`` (``recounts``)."""
        if self.kind not in ("mini", "miniw"):
            raise ValueError("prefetch_plan() is for mini tables")
        if stream.table_valid(False) is not stream.valid or not stream.rows_inside_table:
            return                                               # (soft-masked / quality-masked input: plan inside the count)
        L = _lib.load()
        keep = rows if (rows is not None and rows.shuffle_ok and rows.n_rows <= _lib.MINI_MAX_ROWS) else None
        n_words = stream.n_words
        key = self._plan_key(stream.codes, stream.valid, 0, n_words, keep, False, self.log2_slots, self.log2_bucket)
        need = _lib.check(L.pg_mini_plan_bytes(n_words, self.desc()))
        ws = self._mini_spare if self._mini_spare is not None and self._mini_spare.numel() == need else None
        self._mini_spare = None
        if ws is None:
            # a fresh workspace is allocated ON the side stream: a block the caching allocator hands out there is free of pending
            # work of the current stream (with ``after`` set the side stream does not wait for that stream's tail).  The spare
            # workspace was last read by the count BEFORE the one just enqueued, which every ``after`` event lies behind.
            with torch.cuda.stream(side):
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ws.record_stream(torch.cuda.current_stream(self.device))         # (the count that consumes it runs there)
        # ``after`` = an event recorded before this batch's count was enqueued: the plan then runs BESIDE the count (its kernel
        # is small enough to share the CUs with it) instead of behind it
        if after == "first-pass":
            _lib.check(L.pg_mini_wait_first_pass(side.cuda_stream))   # behind the first scatter pass of the count just enqueued
        elif after is not None:
            side.wait_event(after)
        else:
            side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.device(self.device), torch.cuda.stream(side):
            _lib.check(L.pg_mini_plan(stream.codes.data_ptr(), stream.valid.data_ptr(), 0, n_words, self.desc(),
                                      C.byref(keep.rows_desc) if keep is not None else None, ws.data_ptr(), ws.numel(), side.cuda_stream))
            event = torch.cuda.Event()
            event.record(side)
        ws.record_stream(side)
        self._mini_next = _MiniNext(key, ws, event, keep, (stream.codes, stream.valid))

    def can_shuffle(self, plan: "Plan", window: int, vsize: int) -> bool:
        """can ``abundance_from_records`` build the rows of this plan (instead of table lookups)?"""
        if self.kind in ("mini", "miniw"):
            return self._records is not None and self._records[0] is plan and self._emitted == (int(window), int(vsize))
        return self.has_records_for(plan, vsize)

    def has_records_for(self, plan: "Plan", vsize: int) -> bool:
        return (self._records is not None and self._records[0] is plan and vsize <= _lib.SHUFFLE_MAX_VSIZE
                and self.kind == "hash" and bool(self.log2_bucket))

    def abundance_from_records(self, plan: "Plan", window: int, vsize: int, out: torch.Tensor) -> torch.Tensor:
        """abundance rows by shuffle: bucket-wise LDS lookups of the kept records + row-group scatter + LDS row histograms"""
        if not self.can_shuffle(plan, window, vsize):
            raise RuntimeError("no partition records for these rows: count(stream, rows=plan) first")
        n_words = self._records[1]
        L = _lib.load()
        if self.kind in ("mini", "miniw"):
            plan_ws = self._mini_plan.ws
            with torch.cuda.device(self.device):
                _lib.check(L.pg_mini_abundance_from_emitted(self.desc(), C.byref(plan.rows_desc), vsize, out.data_ptr(), plan_ws.data_ptr(),
                                                            plan_ws.numel(), n_words, self._shuffle_ws.data_ptr(), self._shuffle_ws.numel(),
                                                            _stream_ptr(self.device)))
            self._emitted = None        # the row shuffle reuses the emitted words' buffer
            self._records = None
            return out
        emitted = self._emitted == (int(window), int(vsize))          # the lookup pass already ran inside the count
        sws = self._shuffle_ws if emitted else self._shuffle_workspace_for(n_words, plan.n_rows, vsize)
        fn = L.pg_abundance_from_emitted if emitted else L.pg_abundance_from_records
        with torch.cuda.device(self.device):
            _lib.check(fn(self.desc(), C.byref(plan.rows_desc), window, vsize, out.data_ptr(),
                          self._workspace.data_ptr(), self._workspace.numel(), n_words, sws.data_ptr(), sws.numel(), _stream_ptr(self.device)))
        self._emitted = None            # the row shuffle reuses the emitted words' buffer: they are gone now
        return out

    def abundance_of(self, stream: ReadStream, rows: "Plan | Rows", window: int = 10, vsize: int = 400,
                     out: torch.Tensor | None = None) -> torch.Tensor:
        """abundance rows (int32, n_rows x vsize) of ``rows`` of ``stream`` against this FINISHED table -- loaded, merged, or counted
        from whatever reads: ``count_kmer -g DUMP`` (count_kmer.cpp:55-108; a k-mer the table lacks adds nothing, :87).  The table
        is only read.

        A mini table (13 <= k <= 21) takes the super-k-mer form where the library says it applies (pg_mini_find_applies): the
        stream's row-tagged records go bucket by bucket to workgroups that find their k-mers in the table's slices inside LDS
        (pg_mini_find), then the row shuffle writes the rows; ``rows_form`` is "find".  The rows follow the reference's own rule
        (the strict plane ``stream.valid``) whatever the table was counted with.  Everything else -- other kinds, rows the
        merged lookups do not take, a stream whose scratch would not fit in one piece, PG_MINI_FIND=0 -- goes through the lookup
        kernel (pg_features), as ``features`` always did; ``rows_form`` is "lookup".  The records this table kept from its own
        count are dropped."""
        self._require_counts()
        _require_gpu(stream.codes, "the read stream")
        if stream.device != self.device:
            raise ValueError("stream and table are on different devices")
        plan = rows if isinstance(rows, Plan) else Plan(rows, self.device)
        window, vsize = int(window), int(vsize)
        shape = (plan.n_rows, vsize)
        if out is not None and (tuple(out.shape) != shape or out.dtype != torch.int32 or out.device != self.device):
            raise ValueError(f"out must be an int32 tensor of shape {shape} on {self.device}")
        self._records = None
        self._emitted = None
        L = _lib.load()
        n_words = stream.n_words
        find = (self.kind == "mini" and mini_find_wanted() and plan.shuffle_ok and plan.n_segs > 0 and n_words > 0
                and plan.n_rows <= _lib.MINI_MAX_ROWS and _lib.check(L.pg_mini_find_applies(self.desc(), plan.n_rows, window, vsize)) == 1
                and self._piece_words(n_words, True) is None)
        if find:
            self._require_readable()
            abd = out if out is not None else torch.empty(shape, dtype=torch.int32, device=self.device)      # (every row is overwritten)
            if self._find(stream, plan, window, vsize, abd):
                self.rows_form = "find"
                return abd
            out = abd                                            # (a bucket without a free slot: the lookup form below)
        abd = out.zero_() if out is not None else torch.zeros(shape, dtype=torch.int32, device=self.device)
        self.rows_form = "lookup"
        if plan.n_segs:
            self._require_readable()
            with torch.cuda.device(self.device):
                _lib.check(L.pg_features(stream.codes.data_ptr(), stream.valid.data_ptr(), stream.n_words,
                                         plan.seg_row.data_ptr(), plan.seg_start.data_ptr(), plan.seg_end.data_ptr(), plan.n_segs,
                                         0, None, None, self.desc(), window, vsize, abd.data_ptr(), _stream_ptr(self.device)))
        return abd

    def _find(self, stream: ReadStream, plan: "Plan", window: int, vsize: int, abd: torch.Tensor) -> bool:
        """pg_mini_plan (cached as for a count: the plan depends on the stream, the rows and the geometry only) + pg_mini_find +
        the row shuffle.  False: a k-mer the table lacks met a bucket without a free slot (PG_STATUS_TABLE_FULL from the find
        kernel; the table itself is fine) and nothing was written to ``abd``."""
        L = _lib.load()
        n_words = stream.n_words
        rows_ref = self._rows_ref(plan, stream, False)
        key = self._plan_key(stream.codes, stream.valid, 0, n_words, plan, False, self.log2_slots, self.log2_bucket)
        sp = _stream_ptr(self.device)
        with torch.cuda.device(self.device):
            if self._mini_plan is None or self._mini_plan.key != key:
                self._compute_plan(key, stream, stream.valid, None, 0, n_words, plan, rows_ref, (stream.codes, stream.valid))
            n_records, n_long = self.plan_counts()
            plan_ws = self._mini_plan.ws
            self._mini_optimistic = None
            rec_ws = self._grown("_mini_rec_ws", _lib.check(L.pg_mini_records_bytes(_slack(n_records), self.desc())), shrink=True)
            self._mini_sized_for = (n_words, self.log2_slots, self.log2_bucket)
            sws = self._grown("_shuffle_ws", _lib.check(L.pg_mini_shuffle_bytes_merged(n_words, plan.n_rows, vsize, self.desc())))
            mws = self._grown("_merge_ws", _lib.check(L.pg_mini_merge_words(n_words, _slack(n_records), min(_slack(n_long), _slack(n_records)), self.desc())),
                              dtype=torch.int32)
            _lib.check(L.pg_mini_find(stream.codes.data_ptr(), stream.valid.data_ptr(), 0, n_words, self.desc(), rows_ref,
                                      plan_ws.data_ptr(), plan_ws.numel(), rec_ws.data_ptr(), rec_ws.numel(), window, vsize,
                                      sws.data_ptr(), sws.numel(), mws.data_ptr(), mws.numel(), self.status.data_ptr(), sp))
            st = int(self.status[0].item())
            if st == _lib.STATUS_TABLE_FULL:
                self.status.zero_()
                return False
            self.check_status()
            _lib.check(L.pg_mini_abundance_from_emitted(self.desc(), C.byref(plan.rows_desc), vsize, abd.data_ptr(), plan_ws.data_ptr(),
                                                        plan_ws.numel(), n_words, sws.data_ptr(), sws.numel(), sp))
        return True

    def release_workspaces(self) -> None:
        """give the scratch of the counting pipelines back (record buffers, word buffers, plans: tens of GB at BASELINE sizes); the
        table keeps its counts, the next count allocates again"""
        self._workspace = self._shuffle_ws = self._mini_rec_ws = self._mini_spare = None
        self._merge_ws = self._half_ws = self._depth_ws = None
        self._mini_plan = self._mini_next = None
        self._mini_sized_for = self._mini_optimistic = None
        self._records = self._emitted = self._half = None
        if self.data.is_cuda:
            torch.cuda.empty_cache()

    def check_status(self) -> None:
        """raise what the kernels reported in the status word (include/pangaea_feat.h: PG_STATUS_*).  A count that ran on kept
        workspaces and was refused by the kernels is done again here, silently but for ``recounts`` (see ``count``)."""
        if self.kind == "dense":
            return
        st = int(self.status[0].item())
        if st & _lib.STATUS_BOUNDS:
            raise RuntimeError("a kernel of the checked build was about to store outside its buffer (PG_STATUS_BOUNDS): the results are incomplete")
        if st & _lib.STATUS_PLAN_MISMATCH:
            again = self._mini_optimistic
            if again is not None and self._mini_plan is not None:
                # the count ran on the previous batch's workspaces without waiting for its plan's record counts, and this batch has
                # more records than they hold: nothing was written -- read the counts, size the workspaces, count again
                self._mini_optimistic = None
                self.recounts += 1
                self.status.zero_()
                self.plan_counts()
                self._empty = True
                if again.half:
                    self.count_half(again.stream, again.rows, again.emit, check=False, world=again.world,
                                    lowercase_is_base=again.lowercase_is_base)
                else:
                    self.count(again.stream, again.word_begin, again.word_end, check=False, rows=again.rows, emit=again.emit,
                               lowercase_is_base=again.lowercase_is_base)
                return self.check_status()
            self._mini_plan = None
            raise RuntimeError("the partition plan did not describe this stream (PG_STATUS_PLAN_MISMATCH): nothing was counted")
        if st != 0:
            raise _lib.PangaeaError(_lib.PG_ETABLEFULL, f"hash table with 2^{self.log2_slots} slots is full")

    def merge(self, pairs: torch.Tensor, check: bool = True, pending_ok: bool = False) -> "KmerTable":
        """add (key << 22 | count) pairs (slot format, key = key42(code)), e.g. the compacted table of another GPU"""
        if not pending_ok:
            self._require_counts()
        if self.kind not in ("hash", "mini"):
            raise ValueError("merge() is for hash and mini tables; dense tables are summed with all_reduce")
        pairs = pairs.to(self.device, torch.int64).contiguous()
        if self._empty and self.log2_bucket:
            self.data.zero_()            # a reset() bucketed table is only logically empty
        self._empty = False
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_kmer_merge(pairs.data_ptr(), pairs.numel(), self.desc(), self.status.data_ptr(),
                                                 _stream_ptr(self.device)))
        if check:
            self.check_status()
        return self

    @property
    def n_buckets(self) -> int:
        return 1 << (self.log2_slots - self.log2_bucket) if self.kind in ("hash", "mini", "miniw") and self.log2_bucket else 1

    def bucket_counts(self) -> torch.Tensor:
        """occupied slots per bucket, int64 [n_buckets] -- the segment lengths of ``compact()`` (slot order = bucket order)"""
        self._require_counts()
        if self.kind != "hash":
            raise ValueError("bucket_counts() is for hash tables")
        return (self.data.view(self.n_buckets, -1) != 0).sum(dim=1)

    def merge_parts(self, parts, check: bool = True) -> "KmerTable":
        """add other tables of the SAME geometry, each given as (compact(), bucket_counts()); bucket by bucket inside
        LDS when the buckets are LDS-sized, else with global atomics"""
        self._require_counts()
        parts = [(p.to(self.device, torch.int64), c.to(self.device, torch.int64)) for p, c in parts if p.numel()]
        if not parts:
            return self
        if not (self.kind == "hash" and 0 < self.log2_bucket <= _lib.BUCKET_MAX_LOG2_SLOTS):
            for p, _ in parts:
                self.merge(p, check=False)
        else:
            if self._empty:
                self.data.zero_()
            self._empty = False
            pairs = torch.cat([p for p, _ in parts]).contiguous()
            seg, base = [], 0
            for p, c in parts:
                if c.numel() != self.n_buckets or int(c.sum().item()) != p.numel():
                    raise ValueError("merge_parts: bucket counts do not describe the pairs (different table geometry?)")
                seg.append(torch.cat([c.new_zeros(1), torch.cumsum(c, 0)]) + base)
                base += p.numel()
            seg = torch.stack(seg).contiguous()
            with torch.cuda.device(self.device):
                _lib.check(_lib.load().pg_kmer_merge_bucketed(pairs.data_ptr(), seg.data_ptr(), len(parts), self.desc(),
                                                              self.status.data_ptr(), _stream_ptr(self.device)))
        if check:
            self.check_status()
        return self

    # ---- the exchange step's kernels (dist.exchange_table): fills -> bucket-ordered compaction -> rebuild from all parts

    def _bucketed(self) -> bool:
        return self.kind == "hash" and 0 < self.log2_bucket <= _lib.BUCKET_MAX_LOG2_SLOTS

    def bucket_fill(self) -> torch.Tensor:
        """``bucket_counts()`` by one kernel pass over the table (int64 [n_buckets], on the device)"""
        self._require_counts()
        if not self._bucketed():
            raise ValueError("bucket_fill() is for bucketed hash tables")
        if self._empty:
            self.data.zero_()
            self._empty = False
        fill = torch.empty(self.n_buckets, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_bucket_fill(self.desc(), fill.data_ptr(), _stream_ptr(self.device)))
        return fill

    def compact_into(self, out: torch.Tensor, seg: torch.Tensor) -> None:
        """occupied slots, bucket after bucket, into ``out`` at the offsets ``seg`` (int64 [n_buckets + 1], the exclusive
        scan of ``bucket_fill()``); order inside a bucket is unspecified"""
        self._require_counts()
        if not self._bucketed():
            raise ValueError("compact_into() is for bucketed hash tables")
        _require_gpu(out, "the output")
        assert out.dtype == torch.int64 and out.is_contiguous() and seg.dtype == torch.int64 and seg.numel() == self.n_buckets + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_compact(self.desc(), seg.data_ptr(), out.data_ptr(), _stream_ptr(self.device)))

    def _require_counts(self) -> None:
        if self._deferred is not None:
            raise RuntimeError("this table was counted in deferred form and holds no counts until dist.exchange_table / rebuild_from")

    @property
    def pending(self) -> bool:
        """counted in deferred form: the slots hold nothing until ``rebuild_from`` (``dist.exchange_table``)"""
        return self._deferred is not None

    def deferred_fill(self) -> torch.Tensor:
        return self._deferred[0]

    def deferred_compact_into(self, out: torch.Tensor, seg: torch.Tensor) -> None:
        """the deferred count's entries, bucket after bucket, into ``out`` at the offsets ``seg`` (as ``compact_into``)"""
        fill, n_words = self._deferred
        _require_gpu(out, "the output")
        assert out.dtype == torch.int64 and out.is_contiguous() and seg.dtype == torch.int64 and seg.numel() == self.n_buckets + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_deferred_gather(self.desc(), self._workspace.data_ptr(), self._workspace.numel(), n_words,
                                                      fill.data_ptr(), seg.data_ptr(), out.data_ptr(), _stream_ptr(self.device)))

    @property
    def tag_bits(self) -> int:
        """bits of a key below its bucket id (the exchange sends entries as such tags when they fit 31 bits)"""
        return 42 - (self.log2_slots - self.log2_bucket)

    def deferred_planes_into(self, out: torch.Tensor, tag_elem: torch.Tensor, cnt_elem: torch.Tensor,
                             overflow: torch.Tensor, overflow_count: torch.Tensor) -> None:
        """the deferred count's entries in the 6-byte exchange format: bucket b's tags from element ``tag_elem[b]`` of the
        uint32 view of ``out`` (a byte buffer), its counts from element ``cnt_elem[b]`` of the uint16 view; counts beyond
        0xffff leave their remainder as whole entries in ``overflow`` (``overflow_count``: int64 device counter)"""
        fill, n_words = self._deferred
        _require_gpu(out, "the output")
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert tag_elem.dtype == cnt_elem.dtype == torch.int64 and tag_elem.numel() == cnt_elem.numel() == self.n_buckets
        assert overflow.dtype == torch.int64 and overflow_count.dtype == torch.int64
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_deferred_gather_planes(self.desc(), self._workspace.data_ptr(), self._workspace.numel(), n_words,
                                                             fill.data_ptr(), tag_elem.data_ptr(), cnt_elem.data_ptr(), out.data_ptr(),
                                                             overflow.data_ptr(), overflow_count.data_ptr(), overflow.numel(),
                                                             self.status.data_ptr(), _stream_ptr(self.device)))

    def bucket_fill_range(self, buckets: tuple) -> torch.Tensor:
        """occupied slots of buckets ``[begin, end)`` (int64 [end - begin]); the rest of the table is not read"""
        b0, b1 = buckets
        fill = torch.empty(b1 - b0, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_bucket_fill_range(self.desc(), b0, b1, fill.data_ptr(), _stream_ptr(self.device)))
        return fill

    def compact_planes_range(self, buckets: tuple, out: torch.Tensor, tag_elem: torch.Tensor, cnt_elem: torch.Tensor,
                             overflow: torch.Tensor, overflow_count: torch.Tensor) -> None:
        """buckets ``[begin, end)`` of the table in the 6-byte exchange format (as ``deferred_planes_into``; the element
        indices are per bucket of the range)"""
        b0, b1 = buckets
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert tag_elem.dtype == cnt_elem.dtype == torch.int64 and tag_elem.numel() == cnt_elem.numel() == b1 - b0
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_compact_planes_range(self.desc(), b0, b1, tag_elem.data_ptr(), cnt_elem.data_ptr(), out.data_ptr(),
                                                                 overflow.data_ptr(), overflow_count.data_ptr(), overflow.numel(),
                                                                 self.status.data_ptr(), _stream_ptr(self.device)))

    def mark_rebuilt(self) -> None:
        """every bucket range has been rebuilt: the table holds counts again"""
        self._empty = False
        self._deferred = None

    def rebuild_from_planes(self, buf: torch.Tensor, part_stride: int, cap: int, seg: torch.Tensor, buckets: tuple,
                            in_order: bool = True) -> None:
        """rebuild buckets ``[begin, end)`` from gathered 6-byte planes (``seg`` int64 [n_parts, end - begin + 1], indices
        inside every part's range)"""
        b0, b1 = buckets
        _require_gpu(buf, "the gathered planes")
        assert buf.dtype == torch.uint8 and seg.dtype == torch.int64 and seg.is_contiguous() and seg.shape[1] == b1 - b0 + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_kmer_rebuild_planes_range(buf.data_ptr(), int(part_stride), int(cap), seg.data_ptr(), int(seg.shape[0]),
                                                                self.desc(), b0, b1, self.status.data_ptr(), _stream_ptr(self.device)))
        if in_order and b1 == self.n_buckets:       # ranges rebuilt in another order: the caller calls mark_rebuilt()
            self.mark_rebuilt()

    def rebuild_from(self, pairs: torch.Tensor, seg: torch.Tensor, check: bool = True, buckets: tuple | None = None) -> "KmerTable":
        """replace the table by the merge of ``seg.shape[0]`` bucket-ordered compacted tables of this geometry laid out in
        ``pairs`` (``seg`` int64 [n_parts, n_buckets + 1], absolute offsets): one workgroup per bucket, inside LDS.
        ``buckets`` = (begin, end) rebuilds that bucket range only (``seg`` then [n_parts, end - begin + 1]); the table
        holds counts again once every range has been rebuilt -- the caller's business."""
        if not self._bucketed():
            raise ValueError("rebuild_from() is for bucketed hash tables")
        _require_gpu(pairs, "the pairs")
        b0, b1 = buckets if buckets is not None else (0, self.n_buckets)
        assert pairs.dtype == torch.int64 and seg.dtype == torch.int64 and seg.is_contiguous() and seg.shape[1] == b1 - b0 + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_kmer_rebuild_bucketed_range(pairs.data_ptr(), seg.data_ptr(), int(seg.shape[0]), self.desc(), b0, b1,
                                                                  self.status.data_ptr(), _stream_ptr(self.device)))
        if buckets is None or b1 == self.n_buckets:
            self._empty = False             # (the row-tagged records of this rank's count stay valid: the geometry is the same)
            self._deferred = None
        if check:
            self.check_status()
        return self

    def compact(self) -> torch.Tensor:
        """occupied slots of a hash table as an int64 vector (slot format)"""
        self._require_counts()
        if self.kind not in ("hash", "mini"):
            raise ValueError("compact() is for hash and mini tables")
        step = 1 << 30                       # torch's masked select overflows its 32-bit indexing at 2^31 elements
        if self.data.numel() <= step:
            return self.data[self.data != 0]
        return torch.cat([c[c != 0] for c in self.data.split(step)])

    def occupancy(self) -> float:
        self._require_counts()
        if self.kind in ("wide", "miniw"):
            return float(torch.count_nonzero(self._wide_parts()[0]).item()) / (1 << self.log2_slots)
        if self.kind not in ("hash", "mini"):
            return float("nan")
        return float(torch.count_nonzero(self.data).item()) / self.data.numel()

    def items(self):
        """(codes uint64, counts uint64) sorted by code -- host copies, for tests"""
        self._require_counts()
        if self.kind == "dense":
            t = self.data.cpu().numpy().view(np.uint32)
            codes = np.nonzero(t)[0].astype(np.uint64)
            return codes, t[codes.astype(np.int64)].astype(np.uint64)
        if self.kind in ("wide", "miniw"):
            keys, cnts = self._wide_parts()
            occ = keys != 0
            codes = (keys[occ] - 1).cpu().numpy().view(np.uint64)
            counts = cnts[occ].cpu().numpy().view(np.uint32).astype(np.uint64)
            order = np.argsort(codes)
            return codes[order], counts[order]
        s = self.compact().cpu().numpy().view(np.uint64)
        if self.kind == "mini":
            codes, counts = s >> np.uint64(_lib.HASH_COUNT_BITS), s & np.uint64((1 << _lib.HASH_COUNT_BITS) - 1)
            order = np.argsort(codes)
            return codes[order], counts[order]
        codes, counts = key42_inverse(s >> np.uint64(_lib.HASH_COUNT_BITS)), s & np.uint64((1 << _lib.HASH_COUNT_BITS) - 1)
        order = np.argsort(codes)
        return codes[order], counts[order]

    # ------------------------------------------------------------------ asking a finished table (jellyfish query / histo)

    def _require_readable(self) -> None:
        self._require_counts()
        _require_gpu(self.data, "the table")
        if self._empty and self.log2_bucket and self.kind in ("hash", "mini", "miniw"):
            self.data.zero_()            # a reset() bucketed table is only logically empty

    def query(self, codes) -> torch.Tensor:
        """multiplicity of each given k-mer (``jellyfish query`` on the table of src/feature.py:87): int64 on the table's device,
        0 for a k-mer the table does not hold, -1 for a code with bits at or above 2k.

        ``codes``: an int64 / uint64 tensor ON THE DEVICE (used as it is, no host round trip), a numpy integer array, or a list
        of k-mer strings (``encode_kmers``).  A code is a k-mer in the stream's encoding -- A0 C1 T2 G3, newest character in the
        low bits -- of either strand."""
        self._require_readable()
        if isinstance(codes, torch.Tensor):
            _require_gpu(codes, "the codes")
            if codes.dtype not in (torch.int64, torch.uint64):
                raise TypeError(f"codes must be int64 or uint64 (got {codes.dtype})")
            if codes.device != self.device:
                raise ValueError("codes and table are on different devices")
            c = codes.reshape(-1).contiguous()
        else:
            a = np.asarray(codes)
            if a.dtype.kind in "US" or (a.dtype == object and a.size and isinstance(a.flat[0], (str, bytes))):
                a = encode_kmers([s.decode() if isinstance(s, bytes) else s for s in a.reshape(-1).tolist()], self.k)
            elif a.size == 0:
                a = np.zeros(0, np.uint64)
            elif a.dtype.kind not in "iu":
                raise TypeError(f"codes must be integers or k-mer strings (got {a.dtype})")
            c = torch.from_numpy(np.ascontiguousarray(a.reshape(-1)).astype(np.uint64).view(np.int64)).to(self.device)
        if c.numel() == 0:               # (an empty tensor has no address to give the library)
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        out = torch.empty(c.numel(), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_query(self.desc(), c.data_ptr(), c.numel(), out.data_ptr(), _stream_ptr(self.device)))
        return torch.where(out == -1, -1, out.to(torch.int64) & 0xFFFFFFFF)      # (-1 as int32: PG_QUERY_INVALID)

    def spectrum(self, high: int = 10000) -> np.ndarray:
        """the count spectrum (``jellyfish histo`` on the table of src/feature.py:87,103): int64 [high + 2]; entry c = distinct
        canonical k-mers of multiplicity c for 1 <= c <= high, entry high + 1 = those above, entry 0 = 0.  What one reads to
        choose -s and -v: the k-mers beyond window * vector_size fall into no bin of an abundance row (count_kmer.cpp:86-96)."""
        high = int(high)
        if not 1 <= high <= _lib.SPECTRUM_MAX_HIGH:
            raise ValueError(f"high must lie in [1, {_lib.SPECTRUM_MAX_HIGH}] (got {high})")
        self._require_readable()
        hist = torch.empty(high + 2, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_spectrum(self.desc(), high, hist.data_ptr(), _stream_ptr(self.device)))
        return hist.cpu().numpy()

    # ------------------------------------------------------------------ depth of sequences (jellyfish query -s; contig depth)

    def _plane_for(self, stream: ReadStream, plane) -> torch.Tensor:
        """the validity plane a profile reads the stream with (None: jellyfish's view of a sequence, lower-case bases count)"""
        self._require_readable()
        _require_gpu(stream.codes, "the read stream")
        if stream.device != self.device:
            raise ValueError("stream and table are on different devices")
        plane = stream.lenient_valid() if plane is None else plane
        if plane.dtype != torch.int32 or plane.device != self.device or plane.numel() != stream.n_words:
            raise ValueError(f"plane must be an int32 tensor of the stream's {stream.n_words} words on {self.device}")
        return plane.contiguous()

    def profile(self, stream: ReadStream, start: int = 0, end: int | None = None, plane: torch.Tensor | None = None) -> torch.Tensor:
        """the table's count of the k-mer that starts at each character of ``[start, end)`` of ``stream`` (``jellyfish query -s``
        on the table of src/feature.py:87): int64 on the table's device, 0 for a k-mer the table lacks, -1 where no k-mer
        starts -- one of the k characters is not a base under ``plane``, or fewer than k characters are left in the stream.
        ``plane``: a validity plane of the stream (``stream.valid``: the strict rule); None: ``stream.lenient_valid()``.  The
        table is only read (pg_table_profile)."""
        plane = self._plane_for(stream, plane)
        start, end = int(start), stream.n_chars if end is None else int(end)
        if not 0 <= start <= end <= stream.n_chars:
            raise ValueError(f"[{start}, {end}) is no range of the stream's {stream.n_chars} characters")
        if end == start:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        out = torch.empty(end - start, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_profile(self.desc(), stream.codes.data_ptr(), plane.data_ptr(), stream.n_chars, start, end,
                                                    out.data_ptr(), _stream_ptr(self.device)))
        return torch.where(out == -1, -1, out.to(torch.int64) & 0xFFFFFFFF)      # (-1 as int32: PG_PROFILE_NONE)

    def depth(self, stream: ReadStream, ranges=None, lower: int = 1, plane: torch.Tensor | None = None) -> torch.Tensor:
        """how deep the table covers character ranges of ``stream``: int64 [n, 5] on the table's device, per range the columns
        ``_lib.DEPTH_N_KMERS`` (k-mers that lie inside the range), ``DEPTH_N_PRESENT`` (those with a value above 0), ``DEPTH_SUM``,
        ``DEPTH_MAX`` and ``DEPTH_MEDIAN`` (the lower median, zeros included) of their values -- a k-mer's value is its count in
        the table where that is at least ``lower``, else 0; all five are 0 for a range without k-mers.  A k-mer depth of contigs
        against the reads' table is the kind of number scripts/bin_assembly.sh:43 computes by alignment, not that number.

        ``ranges``: a ``(start, end)`` pair of integer numpy arrays or of int64 tensors on the device (used as they are), a
        ``Rows``, or None: the stream's own runs.  Ranges are independent -- they may overlap, repeat, be unsorted or empty --
        but each must lie inside the stream with start <= end, else ValueError before anything is launched (for device tensors
        that is one reduction and its copy to the host).  ``plane`` as for ``profile``.  The table is only read (pg_table_depth:
        ranges of at most ``_lib.DEPTH_SHORT_MAX`` characters never leave the registers of a wavefront, longer ones keep 4 bytes
        per position in a workspace this table holds until ``release_workspaces``)."""
        plane = self._plane_for(stream, plane)
        lower = int(lower)
        if lower < 1:
            raise ValueError(f"lower must be at least 1 (got {lower})")
        if ranges is None:
            ranges = (stream.run_off[:-1], stream.run_off[1:])
        elif isinstance(ranges, Rows):
            ranges = (ranges.start, ranges.end)
        start, end = ranges
        if isinstance(start, torch.Tensor) or isinstance(end, torch.Tensor):
            if not (isinstance(start, torch.Tensor) and isinstance(end, torch.Tensor)) or start.dtype != torch.int64 or end.dtype != torch.int64:
                raise TypeError("range starts and ends must both be int64 tensors (or both numpy arrays)")
            if start.device != self.device or end.device != self.device:
                raise ValueError("ranges and table are on different devices")
            if start.dim() != 1 or start.shape != end.shape:
                raise ValueError("range starts and ends must be two vectors of one length")
            start, end = start.contiguous(), end.contiguous()
            n = int(start.numel())
            if n:
                ln = end - start
                long_ = ln > _lib.DEPTH_SHORT_MAX
                lo, shortest, hi, n_long, long_pos = torch.stack([start.min(), ln.min(), end.max(), long_.sum(),
                                                                  torch.where(long_, ln - (self.k - 1), 0).sum()]).tolist()
        else:
            a, b = np.asarray(start), np.asarray(end)
            if a.ndim != 1 or a.shape != b.shape:
                raise ValueError("range starts and ends must be two vectors of one length")
            if a.size and (a.dtype.kind not in "iu" or b.dtype.kind not in "iu"):
                raise TypeError(f"range starts and ends must be integers (got {a.dtype}, {b.dtype})")
            a, b = a.astype(np.int64), b.astype(np.int64)
            n = int(a.size)
            if n:
                ln = b - a
                long_ = ln > _lib.DEPTH_SHORT_MAX
                lo, shortest, hi, n_long, long_pos = int(a.min()), int(ln.min()), int(b.max()), int(long_.sum()), int((ln[long_] - (self.k - 1)).sum())
                start, end = torch.from_numpy(a).to(self.device), torch.from_numpy(b).to(self.device)
        if n == 0:
            return torch.zeros((0, 5), dtype=torch.int64, device=self.device)
        if lo < 0 or shortest < 0 or hi > stream.n_chars:
            raise ValueError(f"every range must lie inside the stream's {stream.n_chars} characters with start <= end "
                             f"(smallest start {lo}, largest end {hi}, shortest length {shortest})")
        if n_long > _lib.DEPTH_MAX_LONG:
            raise ValueError(f"{n_long} ranges of more than {_lib.DEPTH_SHORT_MAX} characters: one call takes {_lib.DEPTH_MAX_LONG}")
        L = _lib.load()
        ws = self._grown("_depth_ws", _lib.check(L.pg_table_depth_workspace_bytes(n_long, long_pos)), shrink=True)
        out = torch.empty((n, 5), dtype=torch.int64, device=self.device)
        status = torch.zeros(2, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pg_table_depth(self.desc(), stream.codes.data_ptr(), plane.data_ptr(), stream.n_chars, start.data_ptr(), end.data_ptr(),
                                        n, lower, out.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), _stream_ptr(self.device)))
        if n_long and int(status[0].item()) & _lib.STATUS_DEPTH_WORKSPACE:       # (sized from these very ranges: cannot happen)
            raise RuntimeError("pg_table_depth: the workspace did not hold the long ranges (PG_STATUS_DEPTH_WORKSPACE)")
        return out

    # ------------------------------------------------------------------ reads by their k-mers' counts (kmc_tools filter): readops.py

    FILTER_PIECE_BYTES = fastqtext.PIECE_BYTES     # FASTQ text per piece and input of ``filter_fastq`` (PG_FILTER_PIECE_BYTES overrides)

    read_hits, read_spans, read_corrections, read_depths = readops.read_hits, readops.read_spans, readops.read_corrections, readops.read_depths
    filter_fastq, trim_fastq, correct_fastq, normalize_fastq = readops.filter_fastq, readops.trim_fastq, readops.correct_fastq, readops.normalize_fastq

    # ------------------------------------------------------------------ summing finished tables (jellyfish merge)

    @staticmethod
    def kind_admits(kind: str, k: int) -> bool:
        """may a table of this kind hold k-mers of this size?"""
        lo, hi = {"dense": (1, _lib.DENSE_MAX_K), "hash": (1, _lib.HASH_MAX_K), "wide": (1, _lib.WIDE_MAX_K),
                  "mini": (_lib.MINI_MIN_K, _lib.HASH_MAX_K), "miniw": (_lib.HASH_MAX_K + 1, _lib.WIDE_MAX_K)}.get(kind, (1, 0))
        return lo <= k <= hi

    def _n_occupied(self) -> int:
        """entries the table holds (a host wait)"""
        if self.kind == "dense":
            return int(torch.count_nonzero(self.data).item())
        n = 1 << self.log2_slots
        return int(torch.count_nonzero(self.data[:n]).item())

    def _check_mergeable(self, other: "KmerTable") -> None:
        """what ``add_table`` and ``merged`` refuse, before anything is launched"""
        if not isinstance(other, KmerTable):
            raise TypeError(f"a KmerTable is needed (got {type(other).__name__})")
        if other.k != self.k:
            raise ValueError(f"tables of different k cannot be merged ({self.k} and {other.k})")
        if other.device != self.device:
            raise ValueError(f"tables on different devices cannot be merged ({self.device} and {other.device})")
        _require_gpu(other.data, "the table")
        other._require_counts()

    def add_table(self, other: "KmerTable", check: bool = True) -> "KmerTable":
        """add every count of ``other`` -- any kind, any geometry, the same k and device -- to this table (``jellyfish merge`` over the
        tables of src/feature.py:76-94, two tables at a time): pg_table_merge.  Packed kinds (hash, mini) stop at HASH_COUNT_SAT,
        dense, wide and miniw sum in 32 bits.  ``other`` is only read.  The row records this table kept from its own count no
        longer describe it and are dropped."""
        if other is self:
            raise ValueError("a table cannot be added to itself (merged([t, t]) doubles a table)")
        self._check_mergeable(other)
        self._require_counts()
        if other.data.data_ptr() == self.data.data_ptr():
            raise ValueError("the two tables share their storage")
        self._require_readable()
        other._require_readable()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().pg_table_merge(self.desc(), other.desc(), self.status.data_ptr(), _stream_ptr(self.device)))
        self._empty = False
        self._records = None
        self._emitted = None
        if check:
            self.check_status()
        return self

    @classmethod
    def merged(cls, tables, kind: str | None = None) -> "KmerTable":
        """a fresh table that holds the sum of ``tables`` (``jellyfish merge`` over the tables of src/feature.py:76-94); the sources
        are only read, and one may appear more than once.  ``kind``: the result's kind, the first table's by default.  Where all
        sources are of the wanted kind and of one geometry that the library's aligned form takes (pg_table_merge_aligned_applies:
        mini, or hash in LDS-sized buckets), the result has that geometry and is built bucket by bucket inside LDS
        (``merge_form == "aligned"``); where that does not apply, or a bucket of the union overflows, the result is sized for the
        sum of the sources' entries and every source is added with ``add_table`` (``merge_form == "general"``), in a larger table
        when that one fills up too."""
        tables = list(tables)
        if not tables:
            raise ValueError("merged() needs at least one table")
        first = tables[0]
        if not isinstance(first, KmerTable):
            raise TypeError(f"a KmerTable is needed (got {type(first).__name__})")
        _require_gpu(first.data, "the table")
        first._require_counts()
        for t in tables[1:]:
            first._check_mergeable(t)
        kind = kind or first.kind
        if not cls.kind_admits(kind, first.k):
            raise ValueError(f"{kind!r} tables do not admit k = {first.k}")
        for t in tables:
            t._require_readable()
        L = _lib.load()
        dev = first.device
        if kind == first.kind and len(tables) <= 16 and all(L.pg_table_merge_aligned_applies(first.desc(), t.desc()) == 1 for t in tables):
            # (the kernel overwrites every slot: no clearing)
            out = cls(first.k, kind, torch.empty(1 << first.log2_slots, dtype=torch.int64, device=dev), first.log2_slots, first.log2_bucket)
            srcs = (C.POINTER(_lib.pg_table) * len(tables))(*[C.pointer(t._desc) for t in tables])
            with torch.cuda.device(dev):
                _lib.check(L.pg_table_merge_aligned(out.desc(), srcs, len(tables), out.status.data_ptr(), _stream_ptr(dev)))
            if not int(out.status[0].item()) & _lib.STATUS_TABLE_FULL:
                out._empty = False
                out.merge_form = "aligned"
                out.check_status()
                return out
            del out
        hint = max(1024, sum(t._n_occupied() for t in tables))
        while True:
            out = cls.alloc(first.k, dev, kind, distinct_hint=hint)
            for t in tables:
                out.add_table(t, check=False)
            out.merge_form = "general"
            try:
                out.check_status()
                return out
            except _lib.PangaeaError as e:
                if e.code != _lib.PG_ETABLEFULL or out.kind == "dense" or out.log2_slots >= 40:
                    raise
            del out
            hint *= 2                       # (grow and try again, as counting does)

    # ------------------------------------------------------------------ two finished tables met otherwise than by their sum

    @classmethod
    def combined(cls, a: "KmerTable", b: "KmerTable | None", op: str, kind: str | None = None, lower: int = 1,
                 upper: int | None = None) -> "KmerTable":
        """a fresh table of r(x) for every canonical k-mer x, a and b being the counts the two tables STORE for it (0: absent):
        ``min`` min(a, b); ``max`` max(a, b); ``diff`` a - b where a > b; ``left`` a where b > 0; ``only`` a where b == 0;
        ``keep`` a (``b`` is None: see ``filtered``).  Only lower <= r <= upper is kept (``upper`` None: no bound).  The sources --
        any kinds and geometries, the same k and device; the same table twice is fine -- are only read.  ``kind``: the result's
        kind, ``a``'s by default.  Where both sources are of the wanted kind and of one geometry that the library's aligned form
        takes (pg_table_merge_aligned_applies: mini, or hash in LDS-sized buckets), the result has that geometry and is built bucket
        by bucket inside LDS (pg_table_combine_aligned, ``combine_form == "aligned"``); elsewhere, and when a bucket of an aligned
        ``max`` overflows, the surviving entries leave as items (pg_table_combine_items) and the result is built from them as
        ``from_items`` builds a table, sized for their number and grown while it fills up (``combine_form == "general"``).  A value
        that enters a packed kind (hash, mini) is clamped to HASH_COUNT_SAT, as everywhere."""
        code = _lib.COMBINE_OPS.get(op) if isinstance(op, str) else None
        if code is None:
            raise ValueError(f"unknown op {op!r} (one of {', '.join(_lib.COMBINE_OPS)})")
        if (op == "keep") != (b is None):
            raise ValueError("'keep' takes one table and no other" if op == "keep" else f"{op!r} needs two tables")
        if not isinstance(a, KmerTable):
            raise TypeError(f"a KmerTable is needed (got {type(a).__name__})")
        lower, up = int(lower), -1 if upper is None else int(upper)
        if lower < 1:
            raise ValueError(f"lower must be at least 1 (got {lower})")
        if upper is not None and up < lower:
            raise ValueError(f"upper ({up}) is below lower ({lower})")
        _require_gpu(a.data, "the table")
        a._require_counts()
        if b is not None:
            a._check_mergeable(b)
        kind = kind or a.kind
        if not cls.kind_admits(kind, a.k):
            raise ValueError(f"{kind!r} tables do not admit k = {a.k}")
        a._require_readable()
        if b is not None:
            b._require_readable()
        L = _lib.load()
        dev = a.device
        others = [a] if b is None else [a, b]
        if all(t.kind == kind and L.pg_table_merge_aligned_applies(a.desc(), t.desc()) == 1 for t in others):
            # (the kernel overwrites every slot: no clearing)
            out = cls(a.k, kind, torch.empty(1 << a.log2_slots, dtype=torch.int64, device=dev), a.log2_slots, a.log2_bucket)
            with torch.cuda.device(dev):
                _lib.check(L.pg_table_combine_aligned(out.desc(), a.desc(), None if b is None else b.desc(), code, lower, up,
                                                      out.status.data_ptr(), _stream_ptr(dev)))
            if not int(out.status[0].item()) & _lib.STATUS_TABLE_FULL:      # (only a union can outgrow a bucket)
                out._empty = False
                out.combine_form = "aligned"
                out.check_status()
                return out
            del out
        return cls._combined_general(a, b, op, kind, lower, up)

    @classmethod
    def _combined_general(cls, a: "KmerTable", b: "KmerTable | None", op: str, kind: str, lower: int, up: int) -> "KmerTable":
        """the general form of ``combined`` (arguments already checked; ``up`` < 0: no upper bound)"""
        L = _lib.load()
        dev = a.device
        code = _lib.COMBINE_OPS[op]
        # every launch emits a subset of the entries of the table it streams
        cap = a._n_occupied() + (b._n_occupied() if op == "max" else 0)
        codes = torch.empty(max(1, cap), dtype=torch.int64, device=dev)
        counts = torch.empty(max(1, cap), dtype=torch.int32, device=dev)
        n_out = torch.zeros(1, dtype=torch.int64, device=dev)
        status = torch.zeros(2, dtype=torch.int32, device=dev)
        launches = [(a, b, code)] if op != "max" else [(a, b, code), (b, a, _lib.COMBINE_ONLY)]     # (b's own k-mers: the rest of the union)
        with torch.cuda.device(dev):
            for x, y, c in launches:
                _lib.check(L.pg_table_combine_items(x.desc(), None if y is None else y.desc(), c, lower, up, codes.data_ptr(), counts.data_ptr(),
                                                    cap, n_out.data_ptr(), status.data_ptr(), _stream_ptr(dev)))
        n = int(n_out.item())
        if int(status[0].item()) or n > cap:
            raise RuntimeError(f"pg_table_combine_items emitted {n} items into room for {cap}")
        codes, counts = codes[:n], counts[:n].to(torch.int64) & 0xFFFFFFFF
        hint = max(1024, n)
        while True:
            try:
                out = cls.from_items(a.k, codes, counts, dev, kind, distinct_hint=hint)
                out.check_status()
                break
            except _lib.PangaeaError as e:
                if e.code != _lib.PG_ETABLEFULL or kind == "dense" or hint >= 1 << 39:
                    raise
            hint *= 2                       # (grow and try again, as ``merged`` does)
        out._empty = False
        out.combine_form = "general"
        return out

    def filtered(self, lower: int = 1, upper: int | None = None, kind: str | None = None) -> "KmerTable":
        """a fresh table of this one's k-mers with lower <= count <= upper (``upper`` None: no bound) -- e.g. the solid k-mers as
        the ``-g`` table of count_kmer: ``combined(self, None, "keep", ...)``, through the same two forms"""
        return KmerTable.combined(self, None, "keep", kind=kind, lower=lower, upper=upper)

    def compare(self, other: "KmerTable") -> dict:
        """how much two tables share, from two passes on the GPU (pg_table_compare): ``n_a``, ``n_b`` entries, ``sum_a``, ``sum_b``
        total counts, ``n_shared`` k-mers both hold, ``sum_min`` the sum of min(a, b) over them (ints); ``jaccard`` =
        n_shared / (n_a + n_b - n_shared), ``containment_a`` = n_shared / n_a, ``containment_b`` = n_shared / n_b, ``bray_curtis`` =
        1 - 2 sum_min / (sum_a + sum_b) (floats; a ratio over nothing is 0.0).  Counts are the stored ones."""
        self._check_mergeable(other)
        _require_gpu(self.data, "the table")
        self._require_readable()
        other._require_readable()
        L = _lib.load()
        out = torch.empty(8, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.pg_table_compare(self.desc(), other.desc(), out[:4].data_ptr(), _stream_ptr(self.device)))
            _lib.check(L.pg_table_compare(other.desc(), None, out[4:].data_ptr(), _stream_ptr(self.device)))
        n_a, sum_a, n_shared, sum_min, n_b, sum_b = (int(v) for v in out.cpu().tolist()[:6])

        def ratio(x, y):
            return x / y if y else 0.0
        return {"n_a": n_a, "n_b": n_b, "n_shared": n_shared, "sum_a": sum_a, "sum_b": sum_b, "sum_min": sum_min,
                "jaccard": ratio(n_shared, n_a + n_b - n_shared), "containment_a": ratio(n_shared, n_a), "containment_b": ratio(n_shared, n_b),
                "bray_curtis": 1.0 - 2.0 * sum_min / (sum_a + sum_b) if sum_a + sum_b else 0.0}


def encode_kmers(strings, k: int) -> np.ndarray:
    """uint64 codes of k-mer strings in the stream's encoding: ``(c >> 1) & 3`` over ``ACGT`` (A0 C1 T2 G3, count_tnf.cpp:99), the
    first character highest, the newest (last) in the low two bits.  ValueError for a string of another length than ``k`` or with
    any other character (N, lower case, IUPAC)."""
    strings = list(strings)
    k = int(k)
    if not 1 <= k <= _lib.WIDE_MAX_K:
        raise ValueError(f"k-mer size {k} unsupported (1..{_lib.WIDE_MAX_K})")
    for s in strings:
        if not isinstance(s, str) or len(s) != k:
            raise ValueError(f"{s!r} is not a k-mer of length {k}")
    if not strings:
        return np.zeros(0, np.uint64)
    try:
        chars = np.frombuffer("".join(strings).encode("ascii"), dtype=np.uint8).reshape(-1, k)
    except UnicodeEncodeError:
        chars = np.zeros((len(strings), k), np.uint8)
    bad = ~np.isin(chars, np.frombuffer(b"ACGT", dtype=np.uint8)).all(axis=1)
    if bad.any():
        raise ValueError(f"{strings[int(np.nonzero(bad)[0][0])]!r} holds a character other than A, C, G, T")
    d = ((chars >> 1) & 3).astype(np.uint64)
    codes = np.zeros(len(strings), dtype=np.uint64)
    for j in range(k):
        codes = (codes << np.uint64(2)) | d[:, j]
    return codes


def half_piece_words(free_bytes: int, n_words: int, local_log2_slots: int, local_log2_bucket: int, n_rows: int, world: int):
    """words per piece of an N-rank count half (``KmerTable.count_half``): ``n_words`` (one piece) when everything the rank holds
    across the exchange fits 85 % of ``free_bytes``, fewer when only pieces fit, None when not even pieces do.  Per word of the
    stream: the record workspace (one piece at a time), the merged lookups' 2-byte slots and the records' meta words (kept for every
    piece), the piece plans and the row shuffle's word buffers (two of them when the rows take two scatter passes: more than 2^11
    groups of 64).  Fixed: ``pg_mini_half_bytes`` (entry slabs, occupancy), the exchange's send and receive buffers and both bins
    buffers (at most every local slot is an entry, padded to the longest part), and -- in pieces -- the local slots themselves."""
    rec, slots, words = KmerTable._PIECE_BYTES_PER_WORD
    meta, plan = 4 * 7, 4
    groups = max(1, (int(n_rows) + 63) // 64)
    if (groups - 1).bit_length() > 11:
        words *= 2
    n_slots = 1 << int(local_log2_slots)
    n_buckets = n_slots >> int(local_log2_bucket)
    half = 8 * n_slots + 8 * n_buckets * max(1, (1 << int(local_log2_bucket)) // 64) + 4 * n_buckets
    parts = int(1.04 * n_slots) + 8 * int(world)
    exchange = (8 + 8 + 2 + 2) * parts
    budget = 0.85 * free_bytes
    if (rec + slots + words + plan) * n_words + half + exchange <= budget:
        return int(n_words)
    room = budget - half - exchange - 8 * n_slots - (slots + meta + words + plan) * n_words
    if room <= rec * 4 * _lib.WORD_ALIGN:
        return None
    return max(_lib.WORD_ALIGN, int(room / rec) // _lib.WORD_ALIGN * _lib.WORD_ALIGN)


_KEY_MASK = np.uint64((1 << 42) - 1)


def key42(codes: np.ndarray) -> np.ndarray:
    """the slot key of canonical codes (uint64 < 2^42): the library's pg_key42, a bijection on 42 bits"""
    x = np.asarray(codes, dtype=np.uint64).copy()
    for m in (_lib.KEY42_M1, _lib.KEY42_M2):
        x ^= x >> np.uint64(21)
        x = (x * np.uint64(m)) & _KEY_MASK
    x ^= x >> np.uint64(21)
    return x


def key42_torch(codes: torch.Tensor) -> torch.Tensor:
    """``key42`` of an int64 tensor of codes below 2^42, wherever it lives: int64 products wrap modulo 2^64, of which the low 42
    bits are kept, and every intermediate is non-negative, so the shifts are logical"""
    x = codes.clone()
    for m in (_lib.KEY42_M1, _lib.KEY42_M2):
        x ^= x >> 21
        x = (x * m) & ((1 << 42) - 1)
    x ^= x >> 21
    return x


_DUMP_REASONS = {_lib.DUMP_NO_TAB: "no TAB between k-mer and count", _lib.DUMP_BAD_COUNT: f"the count is not 1 to {_lib.DUMP_MAX_DIGITS} decimal digits",
                 _lib.DUMP_CAPACITY: "more lines than the parser was given room for"}


def _dump_error(path: str, k: int, status: int) -> str:
    """the message for pg_dump_parse's status word: (1-based line << 8) | reason"""
    line, reason = status >> 8, status & 0xFF
    if reason == _lib.DUMP_BAD_LENGTH:
        return f"{path}: dump holds k-mers whose length is not {k} (line {line})"
    return f"{path}: line {line}: {_DUMP_REASONS.get(reason, f'malformed (reason {reason})')}"


def key42_inverse(keys: np.ndarray) -> np.ndarray:
    """canonical codes of slot keys: the xorshifts are involutions on 42 bits, the odd multipliers have inverses mod 2^42"""
    x = np.asarray(keys, dtype=np.uint64).copy()
    for m in (_lib.KEY42_M2, _lib.KEY42_M1):
        x ^= x >> np.uint64(21)
        x = (x * np.uint64(pow(m, -1, 1 << 42))) & _KEY_MASK
    x ^= x >> np.uint64(21)
    return x


def distinct_sketch(stream: ReadStream, k: int, word_begin: int = 0, word_end: int | None = None,
                    lowercase_is_base: bool = False, plane: torch.Tensor | None = None) -> torch.Tensor:
    """HyperLogLog registers (int32 [4096], on the device) of the stream's canonical k-mers.  The elementwise maximum of
    two sketches is the sketch of the union -- how the ranks of a multi-GPU job size their common table.  ``plane``: another
    validity plane than the table's (``ReadStream.union_valid``: what a masked count half holds in its local slots)."""
    _require_gpu(stream.codes, "the read stream")
    dev = stream.device
    regs = torch.zeros(_lib.HLL_REGISTERS, dtype=torch.int32, device=dev)
    word_end = stream.n_words if word_end is None else word_end
    with torch.cuda.device(dev):
        valid = stream.table_valid(lowercase_is_base) if plane is None else plane
        _lib.check(_lib.load().pg_kmer_distinct_sketch(stream.codes.data_ptr(), valid.data_ptr(), word_begin, word_end, k,
                                                       regs.data_ptr(), _stream_ptr(dev)))
    return regs


def sketch_estimate(regs: torch.Tensor) -> int:
    """cardinality estimate of a HyperLogLog sketch (~1.6 % standard error at 4096 registers)"""
    r = regs.cpu().numpy().astype(np.float64)
    m = float(len(r))
    est = (0.7213 / (1.0 + 1.079 / m)) * m * m / np.sum(np.exp2(-r))
    zeros = int((r == 0).sum())
    if est <= 2.5 * m and zeros:
        est = m * math.log(m / zeros)                      # linear counting for small cardinalities
    return int(est)


def estimate_distinct(stream: ReadStream, k: int, word_begin: int = 0, word_end: int | None = None,
                      lowercase_is_base: bool = False) -> int:
    """HyperLogLog estimate of the number of distinct canonical k-mers"""
    return sketch_estimate(distinct_sketch(stream, k, word_begin, word_end, lowercase_is_base))


def count_kmers(stream: ReadStream, k: int, kind: str | None = None, distinct_hint: int | None = None,
                max_log2_slots: int = 36, log2_bucket: int | None = None, rows: "Plan | None" = None,
                emit: tuple | None = None, lowercase_is_base: bool = False, load: float | None = None) -> KmerTable:
    """build the table of one stream; a full hash table is re-built with four times the slots.  ``emit`` = (window,
    vector_size) fuses the lookup pass of the abundance rows into the count where that applies (``KmerTable.count``)."""
    resolved = kind or KmerTable.default_kind(k)
    auto_mini = (kind is None and resolved in ("hash", "wide") and rows is not None and emit is not None and rows.shuffle_ok
                 and rows.n_rows <= _lib.MINI_MAX_ROWS and 1 <= emit[1] <= _lib.SHUFFLE_MAX_VSIZE and emit[0] >= 1
                 and (resolved == "wide" or emit[0] * emit[1] <= _lib.HASH_COUNT_SAT) and _lib.MINI_MIN_K <= k <= _lib.WIDE_MAX_K
                 and os.environ.get("PANGAEA_NO_MINI", "0") in ("", "0"))
    if distinct_hint is None and resolved != "dense":
        # size from a HyperLogLog pass (as cheap as the bucket histogram) instead of guessing the coverage; +10 % covers
        # the estimator's error, load 0.4 leaves room for per-bucket variance
        distinct_hint = max(1 << 13, int(1.1 * estimate_distinct(stream, k, lowercase_is_base=lowercase_is_base)))
        load = 0.4 if load is None else load
    elif load is None:
        load = 0.5
    if auto_mini and log2_bucket is None:
        # one GPU, rows and abundance parameters known: the super-k-mer pipeline (table by minimizer buckets) where its geometry
        # (at most 2^15 buckets of 2^14 slots) holds the table
        want = max(1024, int(distinct_hint / load))
        log2 = max(10, math.ceil(math.log2(want)))
        if KmerTable.mini_applies(k, log2):
            kind = "mini" if k <= _lib.HASH_MAX_K else "miniw"
        elif KmerTable.mini_applies(k, log2 - 1) and distinct_hint <= 0.7 * (1 << (log2 - 1)):
            # the largest geometry (2^16 buckets) at a higher load still beats the other pipelines by far (k = 31, 10 M pairs:
            # 2^29 slots at load 0.45 instead of a 2^30-slot direct table)
            kind = "mini" if k <= _lib.HASH_MAX_K else "miniw"
            load = distinct_hint / float(1 << (log2 - 1))
    table = KmerTable.alloc(k, stream.device, kind, distinct_hint, load=load, log2_bucket=log2_bucket)
    while True:
        try:
            return table.count(stream, rows=rows, emit=emit, lowercase_is_base=lowercase_is_base)
        except _lib.PangaeaError as e:
            if e.code != _lib.PG_ETABLEFULL or table.log2_slots >= max_log2_slots:
                raise
            log2 = min(max_log2_slots, table.log2_slots + 2)
            if table.kind in ("mini", "miniw"):
                lb = min(KmerTable.mini_max_log2_bucket(k), table.log2_bucket + 2)
                del table
                table = (KmerTable.mini_with_slots(k, stream.device, log2, lb) if KmerTable.mini_applies(k, log2, lb)
                         else KmerTable.with_slots(k, stream.device, log2) if k <= _lib.HASH_MAX_K
                         else KmerTable.wide_with_slots(k, stream.device, log2))
                continue
            if table.kind == "wide":
                del table
                table = KmerTable.wide_with_slots(k, stream.device, log2)
                continue
            lb = None if log2_bucket is None else min(log2_bucket + 2, _lib.BUCKET_MAX_LOG2_SLOTS)
            if lb is not None and log2 - lb > _lib.BUCKET_MAX_LOG2_BUCKETS:
                lb = 0
            del table
            table = KmerTable.with_slots(k, stream.device, log2, lb)


# ---------------------------------------------------------------------------------------- workspaces ahead of the data

def prewarm_workspaces(device, n_pairs: int, k: int, vsize: int, read_len: int = 150):
    """Start the allocation of the scratch buffers that the super-k-mer pipeline will ask for, on a helper thread, and return the
    thread (``join()`` it before counting; a data set that turns out larger simply allocates again).

    What a FIRST pass over a data set costs besides its kernels is mostly ``hipMalloc``: record buffers, slot buffer and the row
    shuffle's words are tens of GB at BASELINE sizes (38 GB per 10 M read pairs), their sizes follow from the number of read pairs
    within a few percent, and the ingest -- host threads parsing FASTQ -- leaves the GPU's driver idle meanwhile.  The buffers
    are allocated through torch's caching allocator and given straight back to it: the later requests (same thread or not, same
    stream) are served from those blocks (a larger block is split).  ``pangaea.py`` extracts features once per data set
    (/root/reference/src/pangaea.py:70), so the first pass IS the user's pass.  Only for 13 <= k <= 31 (the pipeline that
    needs the buffers); PANGAEA_PREWARM=0 turns it off."""
    import threading
    if not (_lib.MINI_MIN_K <= k <= _lib.WIDE_MAX_K) or n_pairs <= 0 or os.environ.get("PANGAEA_PREWARM", "1") in ("", "0"):
        return None
    device = torch.device(device)
    if device.type != "cuda":
        return None
    L = _lib.load()
    n_words = (n_pairs * 2 * (read_len + 1) + 31) // 32
    n_words = (n_words + _lib.WORD_ALIGN - 1) // _lib.WORD_ALIGN * _lib.WORD_ALIGN
    m = 13 if k >= 16 else 11                        # (pg_device.hpp: mini_m)
    w = min(k - m + 1, 9)
    records = int(n_words * (32.0 / ((w + 1) / 2.0) + 1.0) * 0.9)     # (k = 21: 6.7 per word; measured 6.45)
    kind = _lib.TABLE_MINI if k <= _lib.HASH_MAX_K else _lib.TABLE_MINI_WIDE
    log2 = (_lib.BUCKET_MAX_LOG2_SLOTS if k <= _lib.HASH_MAX_K else _lib.MINI_WIDE_MAX_LOG2_BUCKET_SLOTS) + 15
    lb = KmerTable.mini_default_log2_bucket(k, log2)
    desc = _lib.pg_table(kind, k, log2, lb, None)
    n_rows = max(1, n_pairs // 100)
    sizes = []
    try:
        sizes.append(_lib.check(L.pg_mini_records_bytes(records, C.byref(desc))))
        sizes.append(_lib.check(L.pg_mini_shuffle_bytes_merged(n_words, n_rows, vsize, C.byref(desc))))
        sizes.append(4 * _lib.check(L.pg_mini_merge_words(n_words, records, records // 2, C.byref(desc))))
    except _lib.PangaeaError:
        return None

    def work():
        try:
            with torch.cuda.device(device):
                held = [torch.empty(int(b), dtype=torch.uint8, device=device) for b in sizes]
                del held
        except RuntimeError:                         # (out of memory: the pipeline will say so itself, with its real sizes)
            pass

    th = threading.Thread(target=work, name="pangaea-prewarm", daemon=True)
    th.start()
    return th


# ---------------------------------------------------------------------------------------- TNF columns

_COLMAP_CACHE: dict = {}


def tnf_ncols(k: int) -> int:
    return _lib.check(_lib.load().pg_tnf_ncols(k))


def tnf_colmap(k: int, device=None):
    """(colmap int16-as-uint16 tensor [4^k], column codes uint32 [ncols])"""
    key = (k, str(device))
    if key not in _COLMAP_CACHE:
        n = tnf_ncols(k)
        colmap = np.zeros(4 ** k, dtype=np.uint16)
        codes = np.zeros(n, dtype=np.uint32)
        _lib.check(_lib.load().pg_tnf_colmap(k, colmap.ctypes.data, codes.ctypes.data))
        t = torch.from_numpy(colmap.view(np.int16))
        _COLMAP_CACHE[key] = (t.to(device) if device is not None else t, codes)
    return _COLMAP_CACHE[key]


# ---------------------------------------------------------------------------------------- rows


def plan_segments(rows: Rows, seg_chars: int = DEFAULT_SEG_CHARS):
    L = _lib.load()
    start = np.ascontiguousarray(rows.start, dtype=np.int64)
    end = np.ascontiguousarray(rows.end, dtype=np.int64)
    n = _lib.check(L.pg_plan_segments(start.ctypes.data, end.ctypes.data, len(start), seg_chars, None, None, None))
    seg_row = np.zeros(n, dtype=np.int32)
    seg_start = np.zeros(n, dtype=np.int64)
    seg_end = np.zeros(n, dtype=np.int64)
    _lib.check(L.pg_plan_segments(start.ctypes.data, end.ctypes.data, len(start), seg_chars, seg_row.ctypes.data,
                                  seg_start.ctypes.data, seg_end.ctypes.data))
    return seg_row, seg_start, seg_end


class Plan:
    """device copy of a row set: its work segments (lookup kernels) and its row ranges (row ids in the partition
    records of the shuffle path); re-usable across launches"""

    def __init__(self, rows: Rows, device, seg_chars: int = DEFAULT_SEG_CHARS):
        r, s, e = plan_segments(rows, seg_chars)
        self.n_rows, self.n_segs = len(rows), len(r)
        self.seg_row = torch.from_numpy(r).to(device)
        self.seg_start = torch.from_numpy(s).to(device)
        self.seg_end = torch.from_numpy(e).to(device)
        start = np.ascontiguousarray(rows.start, dtype=np.int64)
        end = np.ascontiguousarray(rows.end, dtype=np.int64)
        # the shuffle path needs sorted, disjoint, non-empty rows (barcode runs are) and at most 2^22 - 2 of them
        self.shuffle_ok = bool(len(start) and len(start) <= _lib.MAX_ROWS and (end > start).all()
                               and (start[1:] >= end[:-1]).all())
        self.row_start = torch.from_numpy(start).to(device)
        self.row_end = torch.from_numpy(end).to(device)
        self.rows_desc = _lib.pg_rows(self.row_start.data_ptr(), self.row_end.data_ptr(), self.n_rows)


def features(stream: ReadStream, rows: Rows | Plan, k_tnf: int | None = 4, table: KmerTable | None = None,
             window: int = 10, vsize: int = 400, seg_chars: int = DEFAULT_SEG_CHARS,
             out_tnf: torch.Tensor | None = None, out_abd: torch.Tensor | None = None):
    """(tnf int32 [N, D] or None, abd int32 [N, V] or None) on the stream's device.

    tnf[r, c]  = occurrences of the c-th canonical k_tnf-mer in run r            (count_tnf.cpp:78-113)
    abd[r, b]  = k-mer occurrences of run r whose global multiplicity // window == b < vsize
                                                                                 (count_kmer.cpp:55-108)
    """
    _require_gpu(stream.codes, "the read stream")
    dev = stream.device
    plan = rows if isinstance(rows, Plan) else Plan(rows, dev, seg_chars)
    n = plan.n_rows
    tnf = abd = None
    colmap_ptr = None
    if k_tnf:
        colmap, _ = tnf_colmap(k_tnf, dev)
        colmap_ptr = colmap.data_ptr()
        tnf = out_tnf.zero_() if out_tnf is not None else torch.zeros((n, tnf_ncols(k_tnf)), dtype=torch.int32, device=dev)
    shuffle = table is not None and table.can_shuffle(plan, window, vsize)
    if table is not None:
        table._require_counts()
        if table.device != dev:
            raise ValueError("stream and table are on different devices")
        if shuffle:                 # every row is overwritten: no zero fill
            abd = out_abd if out_abd is not None else torch.empty((n, vsize), dtype=torch.int32, device=dev)
        else:
            abd = out_abd.zero_() if out_abd is not None else torch.zeros((n, vsize), dtype=torch.int32, device=dev)
    if tnf is None and abd is None:
        raise ValueError("nothing to compute: give k_tnf and/or a table")
    if plan.n_segs == 0:            # no rows (or only empty ones): the zero-filled matrices are the answer
        return tnf, abd
    if shuffle:
        table.abundance_from_records(plan, window, vsize, abd)
        if tnf is None:
            return tnf, abd
        table = None                         # the lookup kernel below only counts TNF
    elif table is not None and table.kind == "mini" and mini_find_wanted():
        # a finished mini table without records of these rows (loaded, merged, counted from other reads or without rows): its
        # buckets find the k-mers of the stream's records (``abundance_of``; the lookup form where that does not apply)
        table.abundance_of(stream, plan, window, vsize, out=abd)
        if tnf is None:
            return tnf, abd
        table = None
    with torch.cuda.device(dev):
        _lib.check(_lib.load().pg_features(
            stream.codes.data_ptr(), stream.valid.data_ptr(), stream.n_words,
            plan.seg_row.data_ptr(), plan.seg_start.data_ptr(), plan.seg_end.data_ptr(), plan.n_segs,
            k_tnf or 0, colmap_ptr, tnf.data_ptr() if tnf is not None else None,
            table.desc() if table is not None else None, window, vsize,
            abd.data_ptr() if (abd is not None and table is not None) else None, _stream_ptr(dev)))
    return tnf, abd
