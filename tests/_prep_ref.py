"""The rewriting of raw stLFR and TELL-seq read pairs of ``pangaea_amd.prepreads`` restated in plain Python on bytes, for the
tests to compare with: the rules of include/pangaea_feat.h, "Raw stLFR and TELL-seq read pairs brought to the BX:Z: form" -- what
``preprocess_stlfr -n -l`` (preprocess_stlfr.cpp:68-113) and ``preprocess_tellseq`` (preprocess_tellseq.cpp:52-84) write for
well-formed input.  Nothing here is shared with the code under test: ``bytes.find`` and ``bytes.split`` find the barcode."""

NO_AT, NO_PLUS, BAD_INDEX, LONG_TAG, NO_HASH, FEW_FIELDS = 1, 2, 4, 5, 6, 7
MAX_B = 253                      # PG_FASTQ_MAX_TAG - 2


class Malformed(ValueError):
    def __init__(self, file: int, record: int, reason: int):
        super().__init__(f"file {file}: record {record}: reason {reason}")
        self.file, self.record, self.reason = file, record, reason


def contents_of(data: bytes) -> list:
    """the lines of a text without their '\\n'; a last line without newline is a line ('\\r' ends no line)"""
    parts = data.split(b"\n")
    return parts[:-1] + ([parts[-1]] if parts[-1] else [])


def records_of(data: bytes) -> list:
    lines = contents_of(data)
    assert len(lines) % 4 == 0, "the text ends inside a record"
    return [lines[i:i + 4] for i in range(0, len(lines), 4)]


def _check_marks(files: list, u: int) -> None:
    """'@' and '+' of unit u in every file; the error of the first file that has one ('@' before '+')"""
    for f, rec in enumerate(files):
        if not rec[u][0].startswith(b"@"):
            raise Malformed(f, u, NO_AT)
        if not rec[u][2].startswith(b"+"):
            raise Malformed(f, u, NO_PLUS)


def stlfr_plan(h: bytes) -> tuple:
    """(p, B, tagged) of a stLFR header's content: the first '#', the barcode between it and the first '/' behind it (or the end),
    tagged iff neither of the first two '_'-separated fields is the string "0" -- the third is never asked"""
    p = h.find(b"#")
    if p < 0:
        raise Malformed(0, -1, NO_HASH)
    q = h.find(b"/", p + 1)
    B = h[p + 1:] if q < 0 else h[p + 1:q]
    fields = B.split(b"_", 2)
    if len(fields) < 3:
        raise Malformed(0, -1, FEW_FIELDS)
    if len(B) > MAX_B:
        raise Malformed(0, -1, LONG_TAG)
    return p, B, fields[0] != b"0" and fields[1] != b"0"


def tellseq_plan(h: bytes, B: bytes) -> tuple:
    """(s, B, kept): the header up to its first space, kept iff the index read has exactly 18 bytes"""
    s = h.find(b" ")
    return (len(h) if s < 0 else s), B, len(B) == 18


def plan(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None) -> list:
    """per unit (head_len, B, tagged / kept); Malformed with the unit's ordinal for the first malformed unit"""
    files = [records_of(r1), records_of(r2)] + ([records_of(i1)] if short_type == "tellseq" else [])
    assert len({len(x) for x in files}) == 1, "files of different record counts"
    out = []
    for u in range(len(files[0])):
        _check_marks(files, u)
        h = files[0][u][0]
        try:
            out.append(stlfr_plan(h) if short_type == "stlfr" else tellseq_plan(h, files[2][u][1]))
        except Malformed as e:
            raise Malformed(0, u, e.reason) from None
    return out


def preprocess(short_type: str, r1: bytes, r2: bytes, i1: bytes | None = None) -> dict:
    """the files the reference's tool writes: ``out1``, ``out2``, ``wl`` (TELL-seq, else None), and ``pairs``, ``tagged`` (stLFR:
    tagged units; TELL-seq: kept units), ``written`` (units in the output)"""
    plans = plan(short_type, r1, r2, i1)
    recs = [records_of(r1), records_of(r2)]
    outs, wl = [[], []], []
    for u, (head_len, B, flag) in enumerate(plans):
        if short_type == "tellseq" and not flag:
            continue
        header = recs[0][u][0][:head_len] + (b"\tBX:Z:" + B + b"-1" if flag else b"")
        for m in (0, 1):
            third = b"+" if short_type == "tellseq" else recs[m][u][2]
            outs[m].append(b"".join(x + b"\n" for x in (header, recs[m][u][1], third, recs[m][u][3])))
        if short_type == "tellseq":
            wl.append(B + b"\n")
    tagged = sum(1 for x in plans if x[2])
    return {"out1": b"".join(outs[0]), "out2": b"".join(outs[1]), "wl": b"".join(wl) if short_type == "tellseq" else None,
            "units1": outs[0], "units2": outs[1], "pairs": len(plans), "tagged": tagged, "written": len(outs[0])}


def interleaved(res: dict) -> bytes:
    """what ``seqtk mergepe`` makes of the two files: R1's record, then R2's, unit by unit"""
    return b"".join(a + b for a, b in zip(res["units1"], res["units2"]))
