#!/usr/bin/env python3
"""Writes tests/golden/prep/: small raw stLFR and TELL-seq inputs and the files the REFERENCE'S OWN binaries write for them.

    python tests/golden/make_prep_goldens.py DIR_WITH_BINARIES

DIR_WITH_BINARIES holds ``preprocess_stlfr`` and ``preprocess_tellseq`` built from a Pangaea checkout, outside this repository:

    cd src/cpptools && g++ -std=c++11 -I lib/cmdline -I lib/gzstream TOOL.cpp lib/gzstream/gzstream.C -lz -o DIR/TOOL

They are run as the reference's driver runs them (src/run_pangaea:138-162): ``preprocess_stlfr -1 R1 -2 R2 -o PREFIX -n -l`` and
``preprocess_tellseq -1 R1 -2 R2 -l I1 -o PREFIX``.  The inputs are well-formed -- the tools check nothing -- and cover: every
combination of zero and non-zero barcode fields, a barcode without '/', text behind the '/', more '_' in the third field, a '#'
in the read name, a ``+name`` third line, CRLF sequence and quality lines, index reads of 17, 18 and 19 bases and of 18 + '\\r', an
index read with 'N', a header with a tab in front of its space and one without a space; one input set also as gzip."""
import gzip
import os
import subprocess
import sys

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prep")


def rec(header: bytes, seq: bytes, third: bytes = b"+", eol: bytes = b"\n") -> bytes:
    return header + b"\n" + seq + eol + third + eol + b"F" * len(seq) + eol


def stlfr_inputs() -> tuple:
    units = []
    # every tagged / untagged combination of zero fields: f1, f2, f3 each "0" or not
    for i, bc in enumerate([b"5_6_7", b"5_6_0", b"5_0_7", b"5_0_0", b"0_6_7", b"0_6_0", b"0_0_7", b"0_0_0"]):
        units.append((b"@V300%03d" % i + b"L1C001R0010000%d#" % i + bc + b"/1", b"@V300%03d" % i + b"L1C001R0010000%d#" % i + bc + b"/2"))
    units += [
        (b"@nos#12_34_56", b"@nos#12_34_56"),                                       # no '/': the barcode goes to the end
        (b"@behind#12_34_56/1 text behind\tit", b"@behind#12_34_56/2 other"),        # text behind the '/'
        (b"@more#1_2_3_4_5/1", b"@more#1_2_3_4_5/2"),                               # more '_' in f3
        (b"@two#hashes#7_8_9/1", b"@two#hashes#7_8_9/2"),                           # the first '#' wins: B = "hashes#7_8_9"
        (b"@zz#00_0x_10/1", b"@r2 has its own header that is discarded"),           # "00" and "0x" are not "0"
        (b"@empty#__/1", b"@empty#__/2"),                                           # empty fields are not "0"
        (b"@" + b"x" * 80 + b"#1234_5678_9012/1", b"@long/2"),                            # a header of more than 64 bytes
    ]
    r1, r2 = [], []
    for i, (h1, h2) in enumerate(units):
        third = b"+" + h1[1:] if i % 5 == 2 else b"+"                               # a "+name" third line
        eol = b"\r\n" if i % 4 == 1 else b"\n"                                      # CRLF sequence and quality lines
        r1.append(rec(h1, b"ACGTTGCAAC"[:4 + i % 7] * 3, third, eol))
        r2.append(rec(h2, b"TTGACCGTAA"[:3 + i % 5] * 2, b"+", eol))
    return b"".join(r1), b"".join(r2)


def tellseq_inputs() -> tuple:
    index = [b"ACGTACGTACGTACGTAC", b"ACGTACGTACGTACGTA", b"ACGTACGTACGTACGTACG", b"ACGTNCGTACGTACGTNN", b"TTTTTTTTTTTTTTTTTT\r", b"",
             b"GGGGGGGGGGGGGGGGGG", b"ACGTACGTACGTACGTAC", b"CCCCCCCCCCCCCCCCCC", b"AAAAAAAAAAAAAAAAAA"]
    heads = [b"@A00:1:HX:1:1101:1000:2000 1:N:0:ACGT", b"@short17 1:N:0", b"@long19 1:N:0", b"@withN 1:N:0", b"@crlf 1:N:0", b"@empty 1:N:0",
             b"@tab\tbefore the space", b"@nospace", b"@" + b"y" * 62 + b" space at byte 63", b"@two  spaces"]
    r1, r2, i1 = [], [], []
    for i, (h, b) in enumerate(zip(heads, index)):
        third = b"+" + h[1:] if i % 3 == 0 else b"+"
        eol = b"\r\n" if i in (6, 8) else b"\n"
        r1.append(rec(h, b"ACGTTGCAAC" * 2 + b"ACG"[:i % 4], third, eol))
        r2.append(rec(h.replace(b" 1:", b" 2:"), b"TTGACCGTAA" + b"GT"[:i % 3], b"+", eol))
        i1.append(b"@" + h[1:].split(b" ")[0] + b" 1:N:0\n" + b + b"\n+\n" + b"F" * len(b.rstrip(b"\r")) + b"\n")
    return b"".join(r1), b"".join(r2), b"".join(i1)


def main() -> int:
    if len(sys.argv) != 2:
        sys.stderr.write(__doc__)
        return 1
    bins = os.path.abspath(sys.argv[1])
    os.makedirs(HERE, exist_ok=True)

    def put(name: str, data: bytes) -> str:
        path = os.path.join(HERE, name)
        with open(path, "wb") as f:
            f.write(data)
        return path

    s1, s2 = stlfr_inputs()
    p1, p2 = put("stlfr_R1.fq", s1), put("stlfr_R2.fq", s2)
    for name, data in (("stlfr_R1.fq.gz", s1), ("stlfr_R2.fq.gz", s2)):
        with open(os.path.join(HERE, name), "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as z:
            z.write(data)
    subprocess.run([os.path.join(bins, "preprocess_stlfr"), "-1", p1, "-2", p2, "-o", os.path.join(HERE, "stlfr.ref"), "-n", "-l"], check=True,
                   stdout=subprocess.DEVNULL)
    t1, t2, ti = tellseq_inputs()
    p1, p2, pi = put("tellseq_R1.fq", t1), put("tellseq_R2.fq", t2), put("tellseq_I1.fq", ti)
    subprocess.run([os.path.join(bins, "preprocess_tellseq"), "-1", p1, "-2", p2, "-l", pi, "-o", os.path.join(HERE, "tellseq.ref")], check=True,
                   stdout=subprocess.DEVNULL)
    for name in sorted(os.listdir(HERE)):
        print(name, os.path.getsize(os.path.join(HERE, name)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
