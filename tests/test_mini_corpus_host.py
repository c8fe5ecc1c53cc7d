"""The edge-case corpus of tests/_corpus.py and the oracle on it, at every k of the super-k-mer pipeline -- no GPU.

tests/test_mini_corpus_gpu.py compares the kernels with the oracle's table and rows of this corpus, and with themselves under a
reverse complement and a shift of the stream.  What those checks rest on is checked here: the corpus holds what it claims, its
layout puts k-mers across the chunk and round boundaries at every shift, and the ORACLE's table is the same for the reverse
complemented stream and for every shift (rows too)."""
import numpy as np
import pytest

from oracle import oracle

from . import _corpus

KS = list(range(13, 32))


def _same_items(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_revcomp_and_periodic_units():
    assert _corpus.revcomp(b"AACGtN") == b"NaCGTT" and _corpus.revcomp(b"") == b""
    rng = np.random.RandomState(3)
    for p in range(1, 13):
        u = _corpus._unit(rng, p)
        assert len(u) == p and all(u != u[:d] * (p // d) for d in range(1, p) if p % d == 0)


@pytest.mark.parametrize("k", KS)
def test_corpus_holds_what_it_claims(k):
    reads = _corpus.corpus(k)
    assert reads == _corpus.corpus(k) and reads != _corpus.corpus(k, seed=1)              # deterministic, seeded
    half = len(reads) // 2
    fwd = reads[:half]
    assert reads[half:] == [_corpus.revcomp(r) for r in fwd]                               # (f)
    n_a = 2 * k + 41
    assert [len(r) for r in fwd[:n_a]] == list(range(n_a))                                 # (a)
    b, c = fwd[n_a:n_a + 96], fwd[n_a + 96:n_a + 192]
    base = c[0].upper()
    assert len(base) == 96 and set(base) <= set(b"ACGT")
    for j in range(96):                                                                    # (b), (c)
        assert b[j] == base[:j] + b"N" + base[j + 1:]
        low = [i for i in range(96) if c[j][i:i + 1].islower()]
        assert c[j].upper() == base and low == list(range(j, min(96, j + 1 + j % 3)))
    d = fwd[n_a + 192:n_a + 204]
    for p, r in enumerate(d, start=1):                                                     # (d)
        assert len(r) == 150 + p and r == (r[:p] * 200)[:len(r)]
    assert d[0] == b"A" * 151 and d[1].startswith(b"ACAC") and d[2].startswith(b"ACGACG")
    e = fwd[n_a + 204:]
    assert len(e) == 36
    for h, r in zip(range(4, 40), e):                                                      # (e)
        x = r[_corpus.FLANK:_corpus.FLANK + h]
        assert len(r) == 2 * _corpus.FLANK + 2 * h and r[_corpus.FLANK + h:_corpus.FLANK + 2 * h] == _corpus.revcomp(x)
    assert 614 <= len(reads) <= 686


@pytest.mark.parametrize("k", KS)
def test_layout_and_oracle_invariants(k):
    reads = _corpus.corpus(k)
    laid = _corpus.stream_of(reads, 0, k)                                                  # (asserts the layout's own claims)
    n = len(reads)
    assert laid.reads[:n] == reads and laid.reads[n:2 * n] == reads[::-1] and sorted(laid.reads[2 * n:]) == sorted(reads)
    assert laid.reads[2 * n:] != reads and len(laid.names) == len(set(laid.names))
    # a row per read, two in the second copy (but for the reads of 0 and 1 characters and their reverse complements)
    assert np.array_equal(np.bincount(laid.read_of_row), [1] * n + [1 if len(r) < 2 else 2 for r in reads[::-1]] + [1] * n)
    assert len(laid.names) == 4 * n - 4
    rows = laid.rows()
    assert (rows.end > rows.start).all() and (rows.start[1:] == rows.end[:-1]).all() and rows.end[-1] == len(laid.text)
    table = oracle.Table(k, threads=2).count(laid.text)
    _corpus.check_against_oracle(laid, k, table)
    assert 0 < _corpus.n_reads_with_a_kmer(laid, k) < len(laid.reads)
    # the Python count of the records: one per k-mer under a cap of 1 (the abundance rows hold every k-mer of the strict plane
    # once: (10, 400) drops none), fewer under 2, fewest under the cap of this k; records of more than four k-mers need a cap above 4
    m, w, delay, cap = _corpus.mini_geometry(k)
    assert (w, delay) == (k - m + 1, 0) if k <= 21 else w + 2 * delay == k - 12 and 1 <= delay <= 5
    assert cap == {13: 3, 21: 9, 31: 2}.get(k, cap) and 2 <= cap <= 9
    n_kmers = int(laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, 10, 400)).sum())
    by_cap = [_corpus.count_records(laid, k, c) for c in (1, 2, None)]
    assert by_cap[0] == (n_kmers, 0) and by_cap[1][1] == 0 and (by_cap[2][1] > 0) == (cap > 4)
    assert by_cap[0][0] > by_cap[1][0] >= by_cap[2][0] > _corpus.n_reads_with_a_kmer(laid, k)
    # lower-case bases are no bases for the oracle's table, and are bases under jellyfish's rule
    assert _same_items(table.items(), oracle.Table(k).count(laid.text.replace(b"a", b"N").replace(b"c", b"N").replace(b"g", b"N").replace(b"t", b"N")).items())
    lenient = oracle.Table(k).count(laid.text.upper()).items()
    assert np.array_equal(lenient[0], table.items()[0]) and int(lenient[1].sum()) > int(table.items()[1].sum())   # (counts only: (b) holds every k-mer of (c))
    # the reverse complemented stream: the same table
    rc = _corpus.stream_of([_corpus.revcomp(r) for r in reversed(reads)], 0, k)
    assert rc.text != laid.text and _same_items(oracle.Table(k, threads=2).count(rc.text).items(), table.items())
    # every shift against the word grid: the same table, the same rows
    want = laid.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, 1, 64))
    assert (want >= 0).all() and np.array_equal(np.add.reduceat(want, np.flatnonzero(np.diff(laid.read_of_row, prepend=-1))),
                                                np.stack([oracle.abd_row(r, k, table, 1, 64) for r in laid.reads]))
    for j in range(1, 32):
        s = _corpus.stream_of(reads, j, k)
        assert s.text == b"N" * j + laid.text and s.runs[0] == ("", b"N" * j) and s.names == laid.names
        assert np.array_equal(s.start, laid.start + j) and np.array_equal(s.end, laid.end + j)
        assert _same_items(oracle.Table(k, threads=2).count(s.text).items(), table.items())
        if j in (1, 31):
            assert np.array_equal(s.rows_by_oracle(lambda seq: oracle.abd_row(seq, k, table, 1, 64)), want)


# ------------------------------------------------------------------ masks and shards: what tests/test_dist_corpus_gpu.py rests on

SHARDED_KS = list(range(13, 22))
WORLDS = (2, 3)


def _codes_of(text, k):
    return set(oracle.Table(k, threads=2).count(text).items()[0].tolist())


def test_masked_families_and_planes():
    k = 15
    marked = _corpus.masked_corpus(k)
    assert marked == _corpus.masked_corpus(k) and [m.text for m in marked[:len(_corpus.corpus(k))]] == _corpus.corpus(k)
    m = _corpus.Marked(b"ACgTT", (1, 4))
    assert m.revcomp() == _corpus.Marked(b"AAcGT", (0, 3)) and m.revcomp().revcomp() == m
    # only the reads that hold the all-A k-mer are marked among the existing ones, and no clean stretch of them reaches k
    old = [x for x in marked[:len(_corpus.corpus(k))] if x.marks]
    assert sorted(x.text for x in old) == [b"A" * 151, b"T" * 151]
    assert all(np.diff([-1] + list(x.marks) + [len(x.text)]).max() <= k for x in old)
    new = marked[len(_corpus.corpus(k)):]
    assert new[-1] == _corpus.Marked(_corpus.clean_poly_a(k), (), _corpus.COPIES, (2,)) and _corpus.masked_corpus(k, clean_run=False) == marked[:-1]
    half = (len(new) - 1) // 2
    assert new[half:2 * half] == [x.revcomp() for x in new[:half]]
    g = new[:96]
    assert all(x.text == g[0].text and x.marks == (j,) and x.marked_in == (0, 1) for j, x in enumerate(g))
    h = new[96:102]
    assert [len(x.text) for x in h] == list(range(k, k + 6)) and all(x.marks == (len(x.text) // 2,) for x in h)
    for x in new[102:105]:                                                                 # (i): no clean stretch of A or T reaches k
        clean = bytearray(x.text)
        for j in x.marks:
            assert clean[j] in b"AT"
            clean[j] = ord("N")
        assert b"A" * k in x.text and b"T" * k in x.text and b"A" * k not in clean and b"T" * k not in clean
    j_reads = new[105:half]
    assert len(j_reads) == 12 and all(any(c in b"acgt" for c in x.text) and x.marks for x in j_reads)
    assert any(x.text[i:i + 1].islower() for x in j_reads for i in x.marks)                  # a low-quality lower-case base
    # the plane: bit j of word w is character 32 w + j
    mask = np.zeros(70, dtype=bool)
    mask[[0, 31, 33, 69]] = True
    assert _corpus.plane_of(mask, 3).numpy().view(np.uint32).tolist() == [1 | 1 << 31, 2, 1 << 5]
    # the two texts of a small layout
    laid = _corpus.masked_stream_of([_corpus.Marked(b"ACgTACGT", (2, 5), (0, 2))], 3, 4)
    assert laid.text == b"NNN" + b"ACgTACGTN" * 3 and np.flatnonzero(laid.lowq).tolist() == [5, 8, 23, 26]
    assert laid.table_text() == b"NNNACNTANGTNACgTACGTNACNTANGTN" and laid.table_text(True) == b"NNNACNTANGTNACGTACGTNACNTANGTN"


def _classes(sh, lc, k):
    kept, t, r, inside = _corpus.kmer_planes(sh.text, sh.table_text(lc), sh.rows.start, sh.rows.end, k)
    return kept, t, r, inside


@pytest.mark.parametrize("k", SHARDED_KS)
def test_sharded_layouts_meet_the_conditions_of_the_gpu_test(k):
    """tests/test_dist_corpus_gpu.py is vacuous without these: every class of k-mer of the masked rule on every rank, a table-plane
    break at every position of a word, row-only k-mers of all three fates, the all-A k-mer, short reads, partial words at every cut"""
    plain, masked = _corpus.sharded_layout(k, False), _corpus.sharded_layout(k, True)
    without = _corpus.sharded_layout(k, True, clean_run=False)
    for laid in (plain, masked, without):
        assert len(laid.runs[0][1]) % 2 == 1 and laid.runs[0][0] == "" and _corpus.cuts_are_partial(laid, k)
    assert plain.text[len(plain.runs[0][1]):] == _corpus.stream_of(_corpus.corpus(k), 0, k).text
    # rows that leave reads out, in every copy
    n = len(masked.reads) // 3
    has_row = np.zeros(len(masked.reads), dtype=bool)
    has_row[masked.read_of_row] = True
    assert [i for i in range(2 * n, len(masked.reads)) if not has_row[i]] == [i for i in range(2 * n, len(masked.reads)) if i % 5 == 4]
    assert 0 < (~has_row[:n]).sum() < n // 10 and 0 < (~has_row[n:2 * n]).sum() < n // 10
    rows = masked.rows()
    assert (rows.end > rows.start).all() and (rows.start[1:] >= rows.end[:-1]).all() and (rows.start[1:] > rows.end[:-1]).any()
    # the table of the table text: counts on both sides of 64, far below saturation; the all-A k-mer only from the clean run
    table = oracle.Table(k, threads=2).count(masked.table_text())
    _corpus.check_against_oracle(masked, k, table)
    assert table.get(0) == len(_corpus.clean_poly_a(k)) - k + 1 and table.get(0) < 64
    assert 0 not in _codes_of(without.table_text(), k) and 0 not in _codes_of(without.table_text(True), k)
    # a table-plane break between two kept k-mers at every position of a word (whole stream; quality masks, with and without soft masks)
    for lc in (False, True):
        kept, t, r, inside = _corpus.kmer_planes(masked.text, masked.table_text(lc), masked.start, masked.end, k)
        at = np.flatnonzero(kept[1:] & kept[:-1] & (t[1:] != t[:-1])) + 1
        assert {int(p) % 32 for p in at} == set(range(32))
        recs = _corpus.count_records(masked, k, planes=(kept, t, r))
        uncut = _corpus.count_records(masked, k, planes=(kept, np.zeros_like(t), r))
        assert recs[0] > uncut[0] > 0                                                      # (the T cuts make records of their own)
        # a row cut inside a masked record: a row boundary inside a read between two row-only k-mers
        cuts = np.array([int(c) for c, a0 in zip(masked.start, masked.read_start) if c > a0])
        row_only = kept & ~t
        assert (row_only[cuts] & row_only[cuts - 1]).sum() >= 10
    for world in WORLDS:
        cuts = _corpus.run_cuts(masked, world)
        shards = [_corpus.shard(masked, world, rank) for rank in range(world)]
        assert [sh.char_range for sh in shards] == list(zip(cuts[:-1], cuts[1:]))
        assert [sh.row_range[0] for sh in shards[1:]] == [sh.row_range[1] for sh in shards[:-1]] and shards[-1].row_range[1] == len(rows.names)
        counted = [_codes_of(sh.table_text(), k) for sh in shards]
        assert set().union(*counted) == _codes_of(masked.table_text(), k)
        assert [0 in c for c in counted] == [False] * (world - 1) + [True]                   # the all-A k-mer: counted on exactly one rank
        fates, poly_row_only = [], []
        for rank, sh in enumerate(shards):
            # the first and the last word of the shard are partial: _cut_plane masks bits in both (rank 0 begins with the shift's N's)
            assert 0 < sh.hi < 32 and (0 < sh.lo < 32 if rank else sh.text[:32].startswith(masked.runs[0][1]))
            assert sh.stream.n_chars == len(sh.text) and sh.stream.decode() == sh.text.translate(bytes.maketrans(b"acgt", b"NNNN"))
            assert sh.stream.valid_lowq is not None and sh.stream.valid_lower is not None
            got = sh.stream.decode(plane=sh.stream.table_valid(True))
            assert got == sh.table_text(True)
            assert sh.stream.decode(plane=sh.stream.table_valid(False)) == sh.table_text().translate(bytes.maketrans(b"acgt", b"NNNN"))
            assert {k - 1, k, k + 1} <= {len(x) for x in sh.reads}
            for lc in (False, True):
                kept, t, r, inside = _classes(sh, lc, k)
                classes = [t & r & inside, r & ~t & inside, r & ~t & ~inside, ~t & ~r]
                assert all(c[k - 1:].any() for c in classes), (world, rank, lc)
                assert (t & ~r).any() == lc                                                # T and not R: the soft-masked bases alone
            kept, t, r, inside = _classes(sh, False, k)
            mine = _codes_of(_corpus.kmers_at(sh.text, np.flatnonzero(r & ~t & inside), k), k)
            others = set().union(*(c for i, c in enumerate(counted) if i != rank))
            fates.append((bool((mine & others) - counted[rank]), bool(mine & counted[rank]), bool(mine - others - counted[rank])))
            poly_row_only.append(0 in mine)
        assert (True, True, True) in fates and any(poly_row_only[:-1])
    # the plain layout's shards: the same stream as the one-GPU corpus test, a partial word at every cut
    for world in WORLDS:
        for rank in range(world):
            sh = _corpus.shard(plain, world, rank)
            assert 0 < sh.hi < 32 and (0 < sh.lo < 32 or rank == 0) and sh.stream.valid_lowq is None
            assert {k - 1, k, k + 1} <= {len(x) for x in sh.reads}
            assert sh.stream.decode() == sh.text.translate(bytes.maketrans(b"acgt", b"NNNN"))
