"""The barcode sort of ``pangaea_amd.sortreads`` restated in plain Python, for the tests to compare with: the rule of
include/pangaea_feat.h, "Read pairs of a FASTQ text by their barcode tag" -- what src/run_pangaea:237-252 does with awk's
``match($1, /BX:Z:[^[:space:]]+/)`` and ``LANG=C sort -k1,1``, with input order (Python's stable ``sorted``) within one tag.
Nothing here is shared with the code under test: a regular expression over bytes finds the tag, ``sorted`` orders the units."""
import re

TAG = re.compile(rb"BX:Z:[^ \t\n\v\f\r]+")


def lines_of(data: bytes) -> list:
    """the lines of a text with their line ends; a last line without newline is a line"""
    parts = data.split(b"\n")                                # (not splitlines: '\r', '\v' and '\f' end no line)
    return [x + b"\n" for x in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def tag_of(header: bytes):
    """(offset of the match in the header, the match) or (-1, None)"""
    m = TAG.search(header)
    return (m.start(), m.group(0)) if m else (-1, None)


def units_of(data1: bytes, data2: bytes | None = None) -> list:
    """the read pairs of an interleaved text, or of an R1 / R2 pair of texts: each (tag or None, its bytes with a final newline)"""
    l1 = lines_of(data1)
    if data2 is None:
        assert len(l1) % 8 == 0
        blocks = [l1[i:i + 8] for i in range(0, len(l1), 8)]
    else:
        l2 = lines_of(data2)
        assert len(l1) % 4 == 0 and len(l1) == len(l2)
        blocks = [l1[i:i + 4] + l2[i:i + 4] for i in range(0, len(l1), 4)]
    units = []
    for b in blocks:
        body = b"".join(x if x.endswith(b"\n") else x + b"\n" for x in b)
        units.append((tag_of(b[0])[1], body))
    return units


def key(unit) -> tuple:
    """untagged behind tagged; tags as byte strings (Python compares bytes as unsigned bytes, a prefix first)"""
    return (unit[0] is None, unit[0] or b"")


def order(units: list) -> list:
    """the permutation of the stable sort: unit order[i] is the i-th of the output"""
    return sorted(range(len(units)), key=lambda i: key(units[i]))


def sort_text(data1: bytes, data2: bytes | None = None) -> bytes:
    units = units_of(data1, data2)
    return b"".join(units[i][1] for i in order(units))


def runs(units: list) -> int:
    """runs of equal keys in sorted order (the untagged units are one run); 0 for no units"""
    return len({key(u) for u in units})


def barcodes(units: list) -> int:
    """distinct tags"""
    return len({u[0] for u in units if u[0] is not None})


def first_descent(units: list):
    """the ordinal of the first unit that stands before its predecessor, or None"""
    for i in range(1, len(units)):
        if key(units[i]) < key(units[i - 1]):
            return i
    return None
