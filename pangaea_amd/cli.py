"""Command-line faces of the two reference counters, same flags, same output files.

    count_tnf  {-i F | -1 F -2 F} -o OUT.gz [-k 4] [-l 1000] [-t 16]              (count_tnf.cpp:117-125)
    count_kmer {-i F | -1 F -2 F} -g DUMP -o OUT.gz [-k 15] [-l 1000] [-t 16] [-v 400] [-w 10]
                                                                                  (count_kmer.cpp:112-123)
    kmer_table histo {-i F | -1 F -2 F | -g DUMP} -k K [--high 10000] [--full] -o OUT
    kmer_table query {-i F | -1 F -2 F | -g DUMP} -k K [-q FILE] [KMER ...]
    kmer_table dump  {-i F | -1 F -2 F | -g DUMP} -k K [-L LOWER] [-U UPPER] -o OUT
    kmer_table merge -k K [-g DUMP]... [-i F]... [-L LOWER] -o OUT     (two inputs or more; `jellyfish merge` + `dump -c -t`)
    kmer_table combine --op {min,max,diff,left,only} -k K {-ga DUMP | -ia F} {-gb DUMP | -ib F} [-L LOWER] [-U UPPER] -o OUT
    kmer_table compare -k K {-ga DUMP | -ia F} {-gb DUMP | -ib F}      (one JSON line on stdout)
    kmer_table depth {-i F | -1 F -2 F | -g DUMP} -k K -s SEQS.fa[.gz] [-L LOWER] -o OUT.tsv
    kmer_table filter {-g DUMP | -ti F | -t1 F -t2 F} -k K {-i F | -1 F -2 F} [-L LOWER] [-U UPPER] [--min-hits X] [--max-hits X]
                      [--pair any|both|single] [--min-qual-char C] -o OUT [-o2 OUT2]      (one JSON line on stdout)
    kmer_table trim {-g DUMP | -ti F | -t1 F -t2 F} -k K {-i F | -1 F -2 F} [-L LOWER] [-U UPPER] [--mode first|longest] [--min-len N]
                    [--pair any|both|single] [--min-qual-char C] -o OUT [-o2 OUT2]        (one JSON line on stdout)
    kmer_table correct {-g DUMP | -ti F | -t1 F -t2 F} -k K {-i F | -1 F -2 F} [-L LOWER] [-U UPPER] [--min-qual-char C]
                       -o OUT [-o2 OUT2]                                                   (one JSON line on stdout)
    kmer_table normalize {-g DUMP | -ti F | -t1 F -t2 F} -k K {-i F | -1 F -2 F} --target T [--min-depth M] [-L LOWER] [--percentile P]
                         [--pair any|both|single] [--seed S] [--min-qual-char C] -o OUT [-o2 OUT2]  (one JSON line on stdout)
    sort_barcodes {-i F | -1 F -2 F} -o OUT [--short_type {10x,stlfr,tellseq}] [-I INDEX]
                                                                                  (src/run_pangaea:237-252; one JSON line on stdout)
    sort_barcodes --check {-i F | -1 F -2 F} [--short_type ...] [-I INDEX]        (exit status 0: sorted, 1: not; see ``main_sort_barcodes``)
    preprocess_reads --short_type {stlfr,tellseq} -1 R1 -2 R2 [-I INDEX] -o PREFIX (src/run_pangaea:138-162; one JSON line on stdout)
                                                         (what `jellyfish histo` / `jellyfish query` / `jellyfish dump -c -t` give
                                                          from the table the reference keeps on disk, feature.py:87,103; see
                                                          ``main_kmer_table``)
``-t`` is accepted and ignored (the GPU replaces the thread pool).  ``count_kmer -g DUMP``: an existing
jellyfish ``dump -c -t`` file is loaded on the GPU (``KmerTable.from_dump``) with the reference's loader semantics
(count_kmer.cpp:139-170; ``load_dump`` states them on the host and is what the tests compare with); when the
file does not exist the multiplicities are counted on the GPU from the reads themselves, which is what jellyfish
would have reported.  Exit status 0, or 1 on bad arguments / failure, as the reference (cmdline.h:592-597).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        self.print_usage(sys.stderr)
        sys.stderr.write(f"{self.prog}: error: {message}\n")
        raise SystemExit(1)


def _common(prog: str, k_default: int) -> _Parser:
    p = _Parser(prog=prog)
    p.add_argument("-1", "--reads1", default="")
    p.add_argument("-2", "--reads2", default="")
    p.add_argument("-i", "--interleaved", default="")
    p.add_argument("-o", "--output", required=True)
    p.add_argument("-k", "--kmer", type=int, default=k_default)
    p.add_argument("-l", "--len", type=int, default=1000)
    p.add_argument("-t", "--thread", type=int, default=16)
    return p


def _inputs(a):
    if a.interleaved:
        return a.interleaved, None
    if not a.reads1 or not a.reads2:
        sys.stderr.write("Error: --reads1 and --reads2 are needed.\n")
        raise SystemExit(1)
    return a.reads1, a.reads2


def load_dump(path: str, k: int):
    """(canonical codes uint64, counts uint64) of a jellyfish text dump, later lines overriding earlier ones"""
    import pandas as pd
    df = pd.read_csv(path, sep="\t", header=None, names=["kmer", "count"], dtype={"kmer": str, "count": np.int64},
                     keep_default_na=False)
    if len(df) == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    if (df["kmer"].str.len() != k).any():
        raise ValueError(f"{path}: dump holds k-mers whose length is not {k}")
    chars = np.frombuffer("".join(df["kmer"]).encode(), dtype=np.uint8).reshape(-1, k)
    ok = np.isin(chars, np.frombuffer(b"ACGT", dtype=np.uint8)).all(axis=1)
    d = ((chars >> 1) & 3).astype(np.uint64)
    fw = np.zeros(len(df), dtype=np.uint64)
    rc = np.zeros(len(df), dtype=np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | d[:, j]
        rc = rc | ((d[:, j] ^ np.uint64(2)) << np.uint64(2 * j))
    canon = np.minimum(fw, rc)[ok]
    counts = df["count"].to_numpy().astype(np.uint64)[ok]
    # last assignment wins (count_kmer.cpp:166)
    _, last = np.unique(canon[::-1], return_index=True)
    keep = len(canon) - 1 - last
    return canon[keep], counts[keep]


def main_count_tnf(argv=None) -> int:
    a = _common("count_tnf", 4).parse_args(argv)
    r1, r2 = _inputs(a)
    from . import feature
    try:
        names, tnf, _ = feature.compute_features(r1, r2, 0, a.kmer, 1, 1, a.len, want_abd=False)
        feature.write_csv_gz(a.output, names, tnf)
    except Exception as e:
        sys.stderr.write(f"count_tnf: {e}\n")
        return 1
    return 0


def main_count_kmer(argv=None) -> int:
    p = _common("count_kmer", 15)
    p.add_argument("-g", "--global", dest="global_", required=True)
    p.add_argument("-v", "--vector", type=int, default=400)
    p.add_argument("-w", "--window", type=int, default=10)
    a = p.parse_args(argv)
    print(a.interleaved)                       # the reference echoes the interleaved path first (count_kmer.cpp:173)
    r1, r2 = _inputs(a)
    import torch
    from . import feature
    from .kmer import KmerTable
    try:
        table = None
        if os.path.isfile(a.global_):
            # 13 <= k <= 21: a mini table, whose buckets find the k-mers of the reads' super-k-mer records (KmerTable.abundance_of);
            # elsewhere the default kind and the lookup kernel (dense, hash below 13, wide above 21)
            from .kmer import mini_find_wanted
            kind = "mini" if KmerTable.kind_admits("mini", a.kmer) and mini_find_wanted() else None
            table = KmerTable.from_dump(a.global_, a.kmer, torch.device("cuda", torch.cuda.current_device()), kind=kind)
        names, _, abd = feature.compute_features(r1, r2, a.kmer, 0, a.window, a.vector, a.len, want_tnf=False, table=table)
        feature.write_csv_gz(a.output, names, abd)
    except Exception as e:
        sys.stderr.write(f"count_kmer: {e}\n")
        return 1
    return 0


def _table_for(a):
    """the multiplicity table a ``kmer_table`` call asks: loaded from a jellyfish text dump (``-g``), else counted from the reads
    with the table's rule as ``Feature`` applies it (lower-case bases count unless PANGAEA_LOWERCASE_IS_BASE=0; bases of paired
    files below the quality threshold never do)"""
    import torch
    from .kmer import KmerTable
    device = torch.device("cuda", torch.cuda.current_device())
    if a.global_:
        return KmerTable.from_dump(a.global_, a.kmer, device)
    return _counted(a.interleaved or a.reads1, None if a.interleaved else a.reads2, a.kmer, device)


def _counted(r1: str, r2, k: int, device):
    """the table of a FASTQ input (``r2`` None: interleaved), counted with the table's rule as ``_table_for`` states it"""
    from .kmer import count_kmers
    from .reads import ReadStream
    stream = ReadStream.from_fastq(r1, r2, device=device).to(device)
    return count_kmers(stream, k, lowercase_is_base=os.environ.get("PANGAEA_LOWERCASE_IS_BASE", "1") not in ("", "0"))


def _check_window(lower: int, upper) -> None:
    if lower < 1:
        raise ValueError(f"-L must be at least 1 (got {lower})")
    if upper is not None and upper < lower:
        raise ValueError(f"-U ({upper}) is below -L ({lower})")


def _hit_bound_arg(text: str, flag: str):
    """``--min-hits`` / ``--max-hits``: with a '.' a share of the read's k-mers in [0, 1], else a whole number of them"""
    try:
        v = float(text) if "." in text else int(text)
    except ValueError:
        raise ValueError(f"{flag} takes a whole number or, written with a '.', a share in [0, 1] (got {text!r})")
    if v < 0 or (isinstance(v, float) and v > 1.0):
        raise ValueError(f"{flag} {text}: a share lies in [0, 1], a number of k-mers is at least 0")
    return v


def _reads_checks(a, verb: str) -> None:
    """what ``kmer_table filter``, ``kmer_table trim`` and ``kmer_table correct`` refuse alike about k, the table's source, the reads, the outputs, the pair
    rule, the count window and the quality threshold"""
    from . import _lib
    if not 1 <= a.kmer <= _lib.WIDE_MAX_K:
        raise ValueError(f"k-mer size {a.kmer} unsupported (1..{_lib.WIDE_MAX_K})")
    if bool(a.table1) != bool(a.table2):
        raise ValueError("-t1 and -t2 go together")
    if sum((bool(a.global_), bool(a.table_interleaved), bool(a.table1))) > 1:
        raise ValueError(f"{verb} takes the table from one source: -g DUMP, -ti F or -t1 F -t2 F (none: the reads themselves)")
    if bool(a.reads1) != bool(a.reads2):
        raise ValueError("-1 and -2 go together")
    if bool(a.interleaved) == bool(a.reads1):
        raise ValueError(f"the reads to {verb} are -i F or -1 F -2 F (one of the two)")
    if a.reads1 and not a.output2:
        raise ValueError("-1 F -2 F writes two files: -o OUT -o2 OUT2")
    if a.interleaved and a.output2:
        raise ValueError("-o2 goes with -1 F -2 F")
    if a.pair not in ("any", "both", "single"):
        raise ValueError(f"--pair must be any, both or single (got {a.pair!r})")
    if a.pair == "single" and a.reads1:
        raise ValueError("--pair single judges the records of one file; -1 F -2 F is paired")
    if a.lower < 0:
        raise ValueError(f"-L must be at least 0 (got {a.lower})")
    if a.upper is not None and a.upper < a.lower:
        raise ValueError(f"-U ({a.upper}) is below -L ({a.lower})")
    if a.min_qual_char is not None and len(a.min_qual_char) != 1:
        raise ValueError(f"--min-qual-char takes one character (got {a.min_qual_char!r})")


def _reads_sources(a) -> tuple:
    """(table source, reads) of ``kmer_table filter`` / ``trim`` once ``_reads_checks`` has passed: the table source is ("dump",
    path), ("reads", r1, r2 or None) or None (the table of the reads themselves), the reads (r1, r2 or None, out1, out2 or None).
    Nothing is opened but the question whether the inputs exist."""
    reads = (a.interleaved, None, a.output, None) if a.interleaved else (a.reads1, a.reads2, a.output, a.output2)
    for o in reads[2:]:
        if o and o.endswith(".gz"):
            raise ValueError(f"{o}: the kept reads are written as plain text, gzip output is not supported")
    source = ("dump", a.global_) if a.global_ else ("reads", a.table_interleaved, None) if a.table_interleaved else \
        ("reads", a.table1, a.table2) if a.table1 else None
    for f in [x for x in reads[:2] if x] + ([x for x in source[1:] if x] if source else []):
        if not os.path.isfile(f):
            raise ValueError(f"{f}: no such file")
    return source, reads


def _filter_plan(a) -> tuple:
    """the checked arguments of ``kmer_table filter``: (table source, reads, keyword arguments of ``KmerTable.filter_fastq``) -- the
    table source is ("dump", path), ("reads", r1, r2 or None) or None (the table of the reads themselves).  Nothing is opened
    but the question whether the inputs exist."""
    _reads_checks(a, "filter")
    kw = dict(lower=a.lower, upper=a.upper, min_hits=_hit_bound_arg(a.min_hits, "--min-hits"),
              max_hits=None if a.max_hits is None else _hit_bound_arg(a.max_hits, "--max-hits"), pair=a.pair, min_qual_char=a.min_qual_char,
              lowercase_is_base=os.environ.get("PANGAEA_LOWERCASE_IS_BASE", "1") not in ("", "0"))
    source, reads = _reads_sources(a)
    return source, reads, kw


def _trim_plan(a) -> tuple:
    """the checked arguments of ``kmer_table trim``: (table source, reads, keyword arguments of ``KmerTable.trim_fastq``), as
    ``_filter_plan`` gives them.  Nothing is opened but the question whether the inputs exist."""
    _reads_checks(a, "trim")
    if a.mode not in ("first", "longest"):
        raise ValueError(f"--mode must be first or longest (got {a.mode!r})")
    if a.min_len is not None and a.min_len < 1:
        raise ValueError(f"--min-len must be at least 1 (got {a.min_len})")
    kw = dict(lower=a.lower, upper=a.upper, mode=a.mode, min_len=a.min_len, pair=a.pair, min_qual_char=a.min_qual_char,
              lowercase_is_base=os.environ.get("PANGAEA_LOWERCASE_IS_BASE", "1") not in ("", "0"))
    source, reads = _reads_sources(a)
    return source, reads, kw


def _correct_plan(a) -> tuple:
    """the checked arguments of ``kmer_table correct``: (table source, reads, keyword arguments of ``KmerTable.correct_fastq``), as
    ``_trim_plan`` gives them (there is no pair rule: every record is written).  Nothing is opened but the question whether the
    inputs exist."""
    _reads_checks(a, "correct")
    kw = dict(lower=a.lower, upper=a.upper, min_qual_char=a.min_qual_char,
              lowercase_is_base=os.environ.get("PANGAEA_LOWERCASE_IS_BASE", "1") not in ("", "0"))
    source, reads = _reads_sources(a)
    return source, reads, kw


def _normalize_plan(a) -> tuple:
    """the checked arguments of ``kmer_table normalize``: (table source, reads, keyword arguments of ``KmerTable.normalize_fastq``), as
    ``_filter_plan`` gives them (there is no upper count).  Nothing is opened but the question whether the inputs exist."""
    _reads_checks(a, "normalize")
    if a.target is None or a.target < 1:
        raise ValueError(f"--target is the depth to normalise to, a whole number of at least 1 (got {a.target})")
    if a.target >= 1 << 31:
        raise ValueError(f"--target must be below 2^31 (got {a.target})")
    if a.min_depth < 0:
        raise ValueError(f"--min-depth must be at least 0 (got {a.min_depth})")
    if not 0 <= a.percentile <= 100:
        raise ValueError(f"--percentile must lie in 0..100 (got {a.percentile})")
    if not 0 <= a.seed < 1 << 64:
        raise ValueError(f"--seed must lie in [0, 2^64) (got {a.seed})")
    if a.lower < 1:
        raise ValueError(f"-L must be at least 1 (got {a.lower})")
    kw = dict(target=a.target, min_depth=a.min_depth, lower=a.lower, percentile=a.percentile, pair=a.pair, seed=a.seed,
              min_qual_char=a.min_qual_char, lowercase_is_base=os.environ.get("PANGAEA_LOWERCASE_IS_BASE", "1") not in ("", "0"))
    source, reads = _reads_sources(a)
    return source, reads, kw


def _kmer_table_filter(a) -> int:
    """``kmer_table filter``, ``kmer_table trim``, ``kmer_table correct`` and ``kmer_table normalize``: the table from its source, the
    call, one JSON line"""
    import json
    import torch
    from .kmer import KmerTable
    plan = {"trim": _trim_plan, "correct": _correct_plan, "normalize": _normalize_plan}.get(a.cmd, _filter_plan)
    source, (r1, r2, o1, o2), kw = plan(a)
    device = torch.device("cuda", torch.cuda.current_device())
    if source is None:
        table = _counted(r1, r2, a.kmer, device)
    elif source[0] == "dump":
        table = KmerTable.from_dump(source[1], a.kmer, device)
    else:
        table = _counted(source[1], source[2], a.kmer, device)
    call = {"trim": table.trim_fastq, "correct": table.correct_fastq, "normalize": table.normalize_fastq}.get(a.cmd, table.filter_fastq)
    res = call(r1, o1, r2, o2, **kw)
    sys.stdout.write(json.dumps(res) + "\n")
    return 0


_CORRECT_HELP = ("put single-base substitutions in the reads right from a k-mer table and write every read, at the length it came "
                 "with.  The table is loaded from -g DUMP, counted from -ti F or -t1 F -t2 F, or -- no table source -- counted from "
                 "the reads themselves; every k-mer of the reads is then in the table at least once, so that -L 2 or more is what "
                 "makes sense there.")


_NORMALIZE_HELP = ("normalise the read depth from a k-mer table: a read's depth is the --percentile (50: the median) of its k-mers' "
                   "counts, a read -- a pair under --pair any or both, with one draw for both mates -- is kept with probability "
                   "target / depth and dropped when its depth is below --min-depth.  The table is loaded from -g DUMP, counted "
                   "from -ti F or -t1 F -t2 F, or -- no table source, the usual call -- counted from the reads themselves.")


def _kmer_table_parser() -> _Parser:
    """the argument parser of ``main_kmer_table``: one sub-parser per command"""
    p = _Parser(prog="kmer_table")
    sub = p.add_subparsers(dest="cmd", required=True)
    for name in ("histo", "query", "dump", "depth"):
        q = sub.add_parser(name)
        q.add_argument("-1", "--reads1", default="")
        q.add_argument("-2", "--reads2", default="")
        q.add_argument("-i", "--interleaved", default="")
        q.add_argument("-g", "--global", dest="global_", default="")
        q.add_argument("-k", "--kmer", type=int, required=True)
        if name == "histo":
            q.add_argument("--high", type=int, default=10000)
            q.add_argument("--full", action="store_true")
            q.add_argument("-o", "--output", required=True)
        elif name == "dump":
            q.add_argument("-L", "--lower-count", dest="lower", type=int, default=1)
            q.add_argument("-U", "--upper-count", dest="upper", type=int, default=None)
            q.add_argument("-o", "--output", required=True)
        elif name == "depth":
            q.add_argument("-s", "--sequences", required=True)
            q.add_argument("-L", "--lower-count", dest="lower", type=int, default=1)
            q.add_argument("-o", "--output", required=True)
        else:
            q.add_argument("-q", "--queries", default="")
            q.add_argument("kmers", nargs="*")
    q = sub.add_parser("merge")
    q.add_argument("-g", "--global", dest="global_", action="append", default=[])
    q.add_argument("-i", "--interleaved", action="append", default=[])
    q.add_argument("-k", "--kmer", type=int, required=True)
    q.add_argument("-L", "--lower-count", dest="lower", type=int, default=1)
    q.add_argument("-o", "--output", required=True)
    for name in ("combine", "compare"):
        q = sub.add_parser(name)
        q.add_argument("-ga", "--global-a", dest="global_a", default="")
        q.add_argument("-ia", "--interleaved-a", dest="interleaved_a", default="")
        q.add_argument("-gb", "--global-b", dest="global_b", default="")
        q.add_argument("-ib", "--interleaved-b", dest="interleaved_b", default="")
        q.add_argument("-k", "--kmer", type=int, required=True)
        if name == "combine":
            q.add_argument("--op", required=True)
            q.add_argument("-L", "--lower-count", dest="lower", type=int, default=1)
            q.add_argument("-U", "--upper-count", dest="upper", type=int, default=None)
            q.add_argument("-o", "--output", required=True)
    for name in ("filter", "trim", "correct", "normalize"):
        q = sub.add_parser(name, description={"correct": _CORRECT_HELP, "normalize": _NORMALIZE_HELP}.get(name))
        q.add_argument("-g", "--global", dest="global_", default="")
        q.add_argument("-ti", "--table-interleaved", dest="table_interleaved", default="")
        q.add_argument("-t1", "--table-reads1", dest="table1", default="")
        q.add_argument("-t2", "--table-reads2", dest="table2", default="")
        q.add_argument("-k", "--kmer", type=int, required=True)
        q.add_argument("-i", "--interleaved", default="")
        q.add_argument("-1", "--reads1", default="")
        q.add_argument("-2", "--reads2", default="")
        q.add_argument("-L", "--lower-count", dest="lower", type=int, default=1)
        if name == "normalize":
            q.set_defaults(upper=None)                       # (no upper count: what the shared checks read)
        else:
            q.add_argument("-U", "--upper-count", dest="upper", type=int, default=None)
        if name == "filter":
            q.add_argument("--min-hits", dest="min_hits", default="1")
            q.add_argument("--max-hits", dest="max_hits", default=None)
            q.add_argument("--pair", default="any")
        elif name == "trim":
            q.add_argument("--mode", default="longest")
            q.add_argument("--min-len", dest="min_len", type=int, default=None)
            q.add_argument("--pair", default="both")
        elif name == "normalize":
            q.add_argument("--target", type=int, default=None)
            q.add_argument("--min-depth", dest="min_depth", type=int, default=0)
            q.add_argument("--percentile", type=int, default=50)
            q.add_argument("--seed", type=int, default=0)
            q.add_argument("--pair", default="any")
        else:
            q.set_defaults(pair="both")                      # (no pair rule: every record is written; what the shared checks read)
        q.add_argument("--min-qual-char", dest="min_qual_char", default=None)
        q.add_argument("-o", "--output", required=True)
        q.add_argument("-o2", "--output2", default="")
    return p


def _short_type_checks(short_type: str, interleaved: str, index: str, allowed: tuple) -> None:
    """what ``--short_type`` and ``-I`` admit beside each other and beside ``-i``, before any file is looked at (ValueError)"""
    if short_type not in allowed:
        raise ValueError(f"--short_type must be one of {', '.join(allowed)} (got {short_type!r})")
    if short_type == "tellseq" and not index:
        raise ValueError("tellseq reads need their index reads: -I INDEX")
    if short_type != "tellseq" and index:
        raise ValueError(f"-I INDEX goes with --short_type tellseq only, not with {short_type}")
    if short_type != "10x" and interleaved:
        raise ValueError(f"raw {short_type} reads are given as -1 R1 -2 R2, not as -i")


def _sort_plan(a) -> tuple:
    """the checked arguments of ``sort_barcodes``: (src1, src2 or None, out or None).  Nothing is opened but the question whether
    the inputs exist."""
    _short_type_checks(a.short_type, a.interleaved, a.index, ("10x", "stlfr", "tellseq"))
    if bool(a.reads1) != bool(a.reads2):
        raise ValueError("-1 and -2 go together")
    if bool(a.interleaved) == bool(a.reads1):
        raise ValueError("the reads to sort are -i F or -1 F -2 F (one of the two)")
    if a.check and a.output:
        raise ValueError("--check writes nothing: -o does not go with it")
    if not a.check and not a.output:
        raise ValueError("-o OUT is needed (or --check)")
    if a.output and a.output.endswith(".gz"):
        raise ValueError(f"{a.output}: the sorted reads are written as plain text, gzip output is not supported")
    srcs = (a.interleaved, None) if a.interleaved else (a.reads1, a.reads2)
    given = [f for f in srcs + (a.index,) if f]
    if a.output and os.path.realpath(a.output) in {os.path.realpath(f) for f in given}:
        raise ValueError(f"the output must differ from the inputs (got {a.output})")
    for f in given:
        if not os.path.isfile(f):
            raise ValueError(f"{f}: no such file")
    return srcs[0], srcs[1], a.output or None


def main_sort_barcodes(argv=None) -> int:
    """``sort_barcodes {-i F | -1 F -2 F} -o OUT``: the read pairs of the input, plain or gzip, as one interleaved plain FASTQ
    sorted by barcode (``sortreads.sort_fastq``: what step 0 of the reference's driver does, src/run_pangaea:237-252, with input
    order and not read-name order within a barcode); one JSON line on stdout: pairs, barcodes, untagged_pairs, longest_tag,
    passes, already_sorted, bytes, seconds, device_ms per stage.  ``sort_barcodes --check {-i F | -1 F -2 F}``: one JSON line of
    ``sortreads.check_fastq`` -- sorted, first_descent, pairs, barcodes, untagged_pairs -- and exit status 0 when the input is
    sorted, 1 when it is not.  Any failure: a message on stderr and exit status 1 (2 under ``--check``, where 1 has a meaning).
    ``--short_type stlfr`` / ``--short_type tellseq -I INDEX`` (``-1``/``-2`` only): the input is RAW reads of that library, rewritten
    to the ``BX:Z:`` form on the device first (``prepreads``; the JSON line then holds the preprocess counts too); ``10x``, the
    default: barcodes that stand in a ``BX:Z:`` tag already."""
    p = _Parser(prog="sort_barcodes")
    p.add_argument("-1", "--reads1", default="")
    p.add_argument("-2", "--reads2", default="")
    p.add_argument("-i", "--interleaved", default="")
    p.add_argument("-o", "--output", default="")
    p.add_argument("--check", action="store_true")
    p.add_argument("--short_type", default="10x")
    p.add_argument("-I", "--index", default="")
    a = p.parse_args(argv)
    import json
    try:
        src1, src2, out = _sort_plan(a)
        from . import sortreads
        raw = {"short_type": a.short_type, "index": a.index or None} if a.short_type != "10x" else {}
        if a.check:
            res = sortreads.check_fastq(src1, src2, **raw)
            sys.stdout.write(json.dumps(res) + "\n")
            return 0 if res["sorted"] else 1
        sys.stdout.write(json.dumps(sortreads.sort_fastq(src1, out, src2, **raw)) + "\n")
    except Exception as e:
        sys.stderr.write(f"sort_barcodes: {e}\n")
        return 2 if a.check else 1
    return 0


def _prep_plan(a) -> tuple:
    """the checked arguments of ``preprocess_reads``: (R1, R2, index or None, the outputs).  Nothing is opened but the question
    whether the inputs exist."""
    _short_type_checks(a.short_type, "", a.index, ("stlfr", "tellseq"))
    if not a.reads1 or not a.reads2:
        raise ValueError("the raw reads are -1 R1 -2 R2 (both)")
    if a.output.endswith(".gz"):
        raise ValueError(f"{a.output}: the reads are written as plain text (PREFIX_1.fq, PREFIX_2.fq), gzip output is not supported")
    outs = [a.output + "_1.fq", a.output + "_2.fq"] + ([a.output + ".wl"] if a.short_type == "tellseq" else [])
    given = [f for f in (a.reads1, a.reads2, a.index) if f]
    hit = {os.path.realpath(o) for o in outs} & {os.path.realpath(f) for f in given}
    if hit:
        raise ValueError(f"the outputs must differ from the inputs (got {sorted(hit)[0]})")
    for f in given:
        if not os.path.isfile(f):
            raise ValueError(f"{f}: no such file")
    return a.reads1, a.reads2, a.index or None, outs


def main_preprocess_reads(argv=None) -> int:
    """``preprocess_reads --short_type {stlfr,tellseq} -1 R1 -2 R2 [-I INDEX] -o PREFIX``: raw stLFR or TELL-seq reads, plain or
    gzip, as ``PREFIX_1.fq`` / ``PREFIX_2.fq`` with the barcode in a ``BX:Z:`` tag on both mates' headers, and ``PREFIX.wl`` for
    TELL-seq (``prepreads.preprocess_reads``: what the reference's driver does with ``preprocess_stlfr -n -l`` and
    ``preprocess_tellseq``, src/run_pangaea:138-162); one JSON line on stdout: short_type, pairs, tagged_pairs / untagged_pairs or
    kept_pairs / dropped_pairs, bytes, files, seconds, device_ms per stage.  Any failure: a message on stderr and exit status 1."""
    p = _Parser(prog="preprocess_reads")
    p.add_argument("--short_type", required=True)
    p.add_argument("-1", "--reads1", default="")
    p.add_argument("-2", "--reads2", default="")
    p.add_argument("-I", "--index", default="")
    p.add_argument("-o", "--output", required=True)
    a = p.parse_args(argv)
    import json
    try:
        r1, r2, index, _ = _prep_plan(a)
        from . import prepreads
        sys.stdout.write(json.dumps(prepreads.preprocess_reads(a.short_type, r1, r2, a.output, index)) + "\n")
    except Exception as e:
        sys.stderr.write(f"preprocess_reads: {e}\n")
        return 1
    return 0


def main_kmer_table(argv=None) -> int:
    """``kmer_table histo``: the count spectrum, one line ``"<count> <distinct k-mers>"`` for count = 1 .. high + 1 (the last
    line gathers every count above ``--high``); lines of 0 are left out unless ``--full``.  ``kmer_table query``: one line
    ``"<k-mer as given> <count>"`` on stdout per k-mer of the arguments and then of ``-q FILE`` (one per line), in that order;
    either strand may be given, 0 = not in the table.  ``kmer_table dump``: the table as ``jellyfish dump -c -t [-L LOWER]``
    writes it, one line ``"<k-mer>\t<count>"`` per canonical k-mer of count >= LOWER (``KmerTable.write_dump``; the file
    ``count_kmer -g`` and ``kmer_table -g`` read).  The two formats of histo and query follow jellyfish's documented ``histo`` and ``query``
    output; jellyfish is not at hand to compare with, so they are unpinned (like the two rules of DESIGN section 2) -- what the
    tests pin is the content, against the oracle.  ``kmer_table merge``: the sum of two or more inputs -- every ``-g DUMP`` loaded
    as ``-g`` elsewhere, every ``-i FASTQ`` counted as ``-i`` elsewhere, both repeatable -- as one table (``KmerTable.merged``: what
    `jellyfish merge` makes of the tables of feature.py:76-94), written as ``kmer_table dump`` writes it.  ``kmer_table combine``:
    two inputs -- A from ``-ga DUMP`` or ``-ia FASTQ``, B from ``-gb`` or ``-ib``, loaded or counted as ``-g`` / ``-i`` are elsewhere
    -- met by ``--op`` (``KmerTable.combined``: min, max, diff = counts subtracted, left = A's counts of the shared k-mers, only =
    A's k-mers that B lacks), kept where LOWER <= count <= UPPER and written as ``kmer_table dump`` writes a table.  ``kmer_table
    compare``: one JSON line of ``KmerTable.compare`` on the same two inputs.  ``kmer_table dump -U UPPER`` writes only the
    entries of count <= UPPER (``KmerTable.filtered``); without ``-U`` nothing about ``dump`` changes.  ``kmer_table depth``: how
    deep the table covers each sequence of the FASTA file ``-s`` (``ReadStream.from_fasta``, ``KmerTable.depth``; lower-case
    bases are bases, as to ``jellyfish query -s``), one tab-separated line ``name  length  kmers  present  mean  median  max``
    per sequence in file order -- its k-mers, those whose count is at least LOWER, and mean (``%.3f`` of sum / kmers, 0.000
    without k-mers), lower median and maximum of the counts, a count below LOWER taken as 0.  The table comes from exactly one
    of ``-i``, ``-1``/``-2`` and ``-g``.  A k-mer depth beside the alignment depth of scripts/bin_assembly.sh:43, not that number.
    ``kmer_table filter``: the reads of ``-i F`` (mates, if any, interleaved) or ``-1 F -2 F`` whose k-mers the table counts as
    asked, written byte for byte and in input order to ``-o`` (and ``-o2``) as plain FASTQ (``KmerTable.filter_fastq``; what
    `kmc_tools filter` does, beside the read set of scripts/low_abd_reads.sh:10).  The table is loaded from ``-g DUMP``, counted
    from ``-ti F`` or ``-t1 F -t2 F`` as ``-i`` / ``-1 -2`` are elsewhere, or -- no table source -- counted from the reads
    themselves (the usual "drop my own error reads" call).  A read passes iff it has a k-mer and the number h of its k-mers with
    LOWER <= count <= UPPER (``-L`` may be 0: absent k-mers; no ``-U``: no upper bound) satisfies ``--min-hits`` <= h <=
    ``--max-hits``, each a whole number or, written with a '.', a share of the read's k-mers; ``--pair any`` (the default) keeps
    both mates if either passes, ``both`` if both do, ``single`` judges every record of ``-i`` on its own; ``--min-qual-char C``:
    bases of quality below C are no bases.  One JSON line on stdout: records, kept, passed, bases, kmers, hits, seconds, device_ms.
    ``kmer_table trim``: the same reads, table sources and count window, but every written read is CUT to its solid span and not
    copied whole (``KmerTable.trim_fastq``; what `kmc_tools filter -t` and khmer's filter-abund do): a position is solid iff its
    k-mer's count lies in [LOWER, UPPER], ``--mode longest`` (the default) keeps the bases of the longest run of solid positions,
    ``first`` those in front of the first k-mer outside the window; name and ``+`` line stay, sequence and quality are cut alike
    and keep their line ends.  A read passes iff its span has at least ``--min-len`` bases (default K); ``--pair both`` (the
    default here: a mate kept under ``any`` that did not pass is written too, possibly empty), ``any``, ``single`` as for filter.
    One JSON line on stdout: records, kept, passed, trimmed, bases, bases_out, kmers, hits, seconds, device_ms.
    ``kmer_table correct``: the same reads, table sources and count window, but no read is dropped or cut: a base whose k-mers are
    all outside the window, between solid k-mers or between one and an end of the read, is REPLACED when exactly one other base
    makes all of them solid (``KmerTable.correct_fastq``; what khmer, Lighter, BFC and Musket do for single substitutions).
    Every record is written, byte for byte except the corrected bases, so ``-o`` (and ``-o2``) have their inputs' sizes; there is
    no ``--pair``.  Without a table source the table is the reads' own, where every k-mer has count 1 at least: ``-L 2`` or more is
    then what makes sense.  One JSON line on stdout: records, bases, kmers, hits, candidates, corrected, reads_corrected, seconds,
    device_ms.
    ``kmer_table normalize``: the same reads and table sources; coverage normalisation as BBNorm and khmer's normalize-by-median
    do it (``KmerTable.normalize_fastq``).  A read's depth d is the ``--percentile`` (default 50: the lower median) of its k-mers'
    counts in the table, counts below ``-L`` taken as 0 (there is no ``-U``).  Every pair -- every record under ``--pair single`` --
    has one draw w in [0, 2^24) that depends on ``--seed`` and its ordinal alone; a read passes iff it has a k-mer,
    d >= ``--min-depth`` (default 0) and w * d < T * 2^24, i.e. with probability min(1, T / d): what is covered deeper than
    ``--target`` is thinned to about that depth, the rest passes untouched.  ``--pair any`` (the default) keeps a pair at its
    smaller depth, ``both`` at its larger.  Kept records are written byte for byte.  Without a table source the table is the
    reads' own: the usual call.  One JSON line on stdout: records, kept, passed, low, bases, kmers, hits, depth_in, depth_out,
    seconds, device_ms.
    Exit status 0, or 1 with a message on stderr, as ``main_count_kmer``."""
    a = _kmer_table_parser().parse_args(argv)
    from . import _lib
    try:
        if a.cmd in ("filter", "trim", "correct", "normalize"):
            return _kmer_table_filter(a)
        if a.cmd in ("combine", "compare"):
            for side, g, i in (("A", a.global_a, a.interleaved_a), ("B", a.global_b, a.interleaved_b)):
                if bool(g) == bool(i):
                    raise ValueError(f"input {side} is -g{side.lower()} DUMP or -i{side.lower()} FASTQ (one of the two)")
            if not 1 <= a.kmer <= _lib.WIDE_MAX_K:
                raise ValueError(f"k-mer size {a.kmer} unsupported (1..{_lib.WIDE_MAX_K})")
            if a.cmd == "combine":
                if a.op not in ("min", "max", "diff", "left", "only"):
                    raise ValueError(f"--op must be one of min, max, diff, left, only (got {a.op!r})")
                _check_window(a.lower, a.upper)
            import torch
            from .kmer import KmerTable
            device = torch.device("cuda", torch.cuda.current_device())
            A, B = (KmerTable.from_dump(g, a.kmer, device) if g else _counted(i, None, a.kmer, device)
                    for g, i in ((a.global_a, a.interleaved_a), (a.global_b, a.interleaved_b)))
            if a.cmd == "compare":
                import json
                sys.stdout.write(json.dumps(A.compare(B)) + "\n")
            else:
                KmerTable.combined(A, B, a.op, lower=a.lower, upper=a.upper).write_dump(a.output)
            return 0
        if a.cmd == "merge":
            if len(a.global_) + len(a.interleaved) < 2:
                raise ValueError("merge needs two inputs or more (-g DUMP and -i FASTQ, both repeatable)")
            if not 1 <= a.kmer <= _lib.WIDE_MAX_K:
                raise ValueError(f"k-mer size {a.kmer} unsupported (1..{_lib.WIDE_MAX_K})")
            if a.lower < 1:
                raise ValueError(f"-L must be at least 1 (got {a.lower})")
            import torch
            from .kmer import KmerTable
            device = torch.device("cuda", torch.cuda.current_device())
            tables = [KmerTable.from_dump(g, a.kmer, device) for g in a.global_] + [_counted(f, None, a.kmer, device) for f in a.interleaved]
            KmerTable.merged(tables).write_dump(a.output, a.lower)
            return 0
        if not (a.global_ or a.interleaved or (a.reads1 and a.reads2)):
            raise ValueError("no input: -i F, -1 F -2 F or -g DUMP is needed")
        if not 1 <= a.kmer <= _lib.WIDE_MAX_K:
            raise ValueError(f"k-mer size {a.kmer} unsupported (1..{_lib.WIDE_MAX_K})")
        if a.cmd == "depth":
            if sum((bool(a.global_), bool(a.interleaved), bool(a.reads1 or a.reads2))) != 1:
                raise ValueError("depth takes the table from one source: -i F, -1 F -2 F or -g DUMP")
            if a.lower < 1:
                raise ValueError(f"-L must be at least 1 (got {a.lower})")
            if not os.path.isfile(a.sequences):
                raise ValueError(f"{a.sequences}: no such sequence file")
            from .reads import ReadStream
            table = _table_for(a)
            seqs = ReadStream.from_fasta(a.sequences, device=table.device)
            d = table.depth(seqs, lower=a.lower).cpu().numpy()
            lengths = np.diff(seqs.run_off) - 1              # (every run ends with the one 'N' that from_fasta appends)
            with open(a.output, "w") as f:
                f.writelines(f"{name}\t{int(n)}\t{int(r[0])}\t{int(r[1])}\t{(int(r[2]) / int(r[0]) if r[0] else 0.0):.3f}\t{int(r[4])}\t{int(r[3])}\n"
                             for name, n, r in zip(seqs.run_names, lengths, d))
        elif a.cmd == "histo":
            if not 1 <= a.high <= _lib.SPECTRUM_MAX_HIGH:
                raise ValueError(f"--high must lie in [1, {_lib.SPECTRUM_MAX_HIGH}]")
            hist = _table_for(a).spectrum(a.high)
            with open(a.output, "w") as f:
                f.writelines(f"{c} {int(hist[c])}\n" for c in range(1, a.high + 2) if a.full or hist[c])
        elif a.cmd == "dump":
            _check_window(a.lower, a.upper)
            if a.upper is None:
                _table_for(a).write_dump(a.output, a.lower)
            else:
                _table_for(a).filtered(a.lower, a.upper).write_dump(a.output)
        else:
            from .kmer import encode_kmers
            asked = list(a.kmers)
            if a.queries:
                with open(a.queries) as f:
                    asked += [line.strip() for line in f if line.strip()]
            codes = encode_kmers(asked, a.kmer)              # a bad k-mer is refused before anything is counted
            counts = _table_for(a).query(codes).cpu().numpy() if asked else []
            sys.stdout.writelines(f"{s} {int(c)}\n" for s, c in zip(asked, counts))
    except Exception as e:
        sys.stderr.write(f"kmer_table: {e}\n")
        return 1
    return 0
