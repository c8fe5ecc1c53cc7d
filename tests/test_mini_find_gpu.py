"""Abundance rows against a FINISHED mini table in super-k-mer form: ``KmerTable.abundance_of`` (pg_mini_find: the bucket workgroup
that finds instead of inserting) -- what ``count_kmer -g DUMP`` computes (cpptools/count_kmer.cpp:55-108; a k-mer the table does not
hold adds nothing, :87).

Integer results, compared exactly.  The expected rows always come from the oracle: ``oracle.abd_row(text of the row, k, table, window,
vsize)`` per row, the table made by ``oracle.Table(k).count(text)`` or by ``.set`` for chosen counts.  Read sets are synthetic, a few
hundred pairs in 3 to 20 barcodes, with N's; what the cases rest on (how many of the looked-up k-mers the table holds, how full its
buckets are) is asserted on the oracle or on the table before the lookups run.  Every form leaves the table bit-identical (``_rows``)."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, cli, feature, kmer, synth
from pangaea_amd.reads import ReadStream

from .conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAT = _lib.HASH_COUNT_SAT


@functools.lru_cache(maxsize=None)
def _runs(seed, n_pairs=300, n_barcodes=7):
    """[(barcode, text)] of a synthetic read set: reads of 150 characters, each followed by a non-base"""
    cfg = synth.SynthConfig(n_pairs=n_pairs, n_barcodes=n_barcodes, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2,
                            seed=seed)
    s = synth.generate(cfg, device="cpu")
    text = s.decode()
    return tuple((name, text[a:b]) for name, a, b in zip(s.run_names, s.run_off[:-1], s.run_off[1:]))


def _second_half_plus(a_runs, c_runs):
    """B: the second half of A's runs followed by as many runs of another genome set (barcodes renamed: every run a row of its own)"""
    half = a_runs[len(a_runs) // 2:]
    return tuple((f"h{i}", t) for i, (_, t) in enumerate(half)) + tuple((f"c{i}", t) for i, (_, t) in enumerate(c_runs[1:1 + len(half)]))


def _text(runs):
    return b"".join(t for _, t in runs)


def _otable(k, *texts):
    t = oracle.Table(k, threads=4)
    for x in texts:
        t.count(x)
    return t


def _share(k, table, text):
    """fraction of the distinct k-mers of ``text`` that ``table`` holds"""
    mine = oracle.Table(k, threads=4).count(text).items()[0]
    return float(np.isin(mine, table.items()[0]).mean())


def _stream(runs):
    return ReadStream.from_runs(list(runs), device=DEV)


def _want(s, rows, k, otab, window, vsize):
    text = s.decode()
    return np.stack([oracle.abd_row(text[a:b], k, otab, window, vsize) for a, b in zip(rows.start, rows.end)])


def _rows(table, s, plan, window=10, vsize=400, form="find", **kw):
    """``table.abundance_of`` with the checks every case shares: the form taken, and a table that is bit-identical afterwards"""
    before = table.data.clone()
    abd = table.abundance_of(s, plan, window, vsize, **kw)
    assert table.rows_form == form
    assert torch.equal(table.data, before)
    assert abd.dtype == torch.int32 and tuple(abd.shape) == (plan.n_rows, vsize)
    assert int(table.status[0].item()) == 0
    return abd.cpu().numpy()


def _same_items(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _mini(k, log2_slots, log2_bucket, s):
    return kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket).count(s)


# 1 ---- same reads: the find form against the fused count + lookups and the oracle; every CAP class and window (k = 13 .. 21), the
# 512- and 1024-thread geometries, tables without a second scatter pass (64 buckets, one bucket)
@pytest.mark.parametrize("k,log2_slots,log2_bucket,n_pairs", [(k, 20, 10, 300) for k in range(13, 22)]
                         + [(21, 20, 12, 300), (21, 20, 13, 300), (21, 24, 14, 300), (21, 20, 14, 300), (21, 14, 14, 24)])
def test_same_reads_equal_the_fused_rows_and_the_oracle(k, log2_slots, log2_bucket, n_pairs):
    runs = _runs(500 + k, n_pairs, 7 if n_pairs > 100 else 3)
    s = _stream(runs)
    rows = s.rows(302)
    plan = kmer.Plan(rows, DEV)
    fused = kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket).count(s, rows=plan, emit=(10, 400))
    assert fused.can_shuffle(plan, 10, 400)
    _, abd_fused = kmer.features(s, plan, k_tnf=None, table=fused, window=10, vsize=400)
    t = _mini(k, log2_slots, log2_bucket, s)
    assert _same_items(t.items(), fused.items()) and not t.can_shuffle(plan, 10, 400)
    abd = _rows(t, s, plan)
    assert np.array_equal(abd, abd_fused.cpu().numpy())
    assert np.array_equal(abd, _want(s, rows, k, _otable(k, _text(runs)), 10, 400))
    # ... and again with the cached plan, into a given matrix
    out = torch.full((plan.n_rows, 400), -7, dtype=torch.int32, device=DEV)
    plan_ws = t._mini_plan.ws
    assert np.array_equal(_rows(t, s, plan, out=out), abd) and t._mini_plan.ws is plan_ws
    assert np.array_equal(out.cpu().numpy(), abd)


# 2 ---- other reads: the table is A's, the rows are B's -- about half of B's k-mers are absent
@pytest.mark.parametrize("k", [15, 21])
@pytest.mark.parametrize("window,vsize", [(10, 400), (1, 6)])
def test_other_reads(k, window, vsize):
    a, c = _runs(500 + k), _runs(900 + k)
    b = _second_half_plus(a, c)
    otab = _otable(k, _text(a))
    assert 0.25 <= _share(k, otab, _text(b)) <= 0.75
    sb = _stream(b)
    rows = sb.rows(302)
    want = _want(sb, rows, k, otab, window, vsize)
    t = _mini(k, 20, 10, _stream(a))
    assert np.array_equal(_rows(t, sb, kmer.Plan(rows, DEV), window, vsize), want)
    assert want.sum() > 0


# 3 ---- nothing shared: every probe ends at an empty slot
def test_nothing_shared():
    k = 21
    a, c = _runs(500 + k), _runs(900 + k)
    otab = _otable(k, _text(a))
    assert _share(k, otab, _text(c)) == 0.0
    sc = _stream(c)
    plan = kmer.Plan(sc.rows(302), DEV)
    t = _mini(k, 20, 10, _stream(a))
    assert not _rows(t, sc, plan).any()


# 4 ---- chosen counts: bin edges, counts beyond the vector (dropped), saturated counts
@pytest.mark.parametrize("k,window,vsize", [(15, 10, 400), (21, 3, 64)])
def test_chosen_counts(k, window, vsize):
    b = _second_half_plus(_runs(500 + k), _runs(900 + k))
    codes = oracle.Table(k, threads=4).count(_text(b)).items()[0]
    rs = np.random.RandomState(k)
    counts = rs.randint(0, window * vsize + 51, size=len(codes)).astype(np.int64)
    edges = np.array([0, 1, window - 1, window, window + 1, window * vsize - 1, window * vsize, window * vsize + 1, SAT - 1, SAT, SAT, SAT])
    counts[rs.choice(len(codes), size=len(edges), replace=False)] = edges
    # (a packed table does not keep an entry of count 0 -- from_items drops it --: such a k-mer is absent, for the oracle too)
    otab = oracle.Table(k)
    for code, n in zip(codes[counts > 0].tolist(), counts[counts > 0].tolist()):
        otab.set(code, n)
    t = kmer.KmerTable.from_items(k, codes, counts, DEV, kind="mini")
    assert t.kind == "mini" and np.array_equal(t.items()[0], codes[counts > 0])
    sb = _stream(b)
    rows = sb.rows(302)
    want = _want(sb, rows, k, otab, window, vsize)
    got = _rows(t, sb, kmer.Plan(rows, DEV), window, vsize)
    assert np.array_equal(got, want)
    # some occurrences were dropped (no entry, beyond the vector, saturated), and the first and the last bin are in use
    ones = oracle.Table(k)
    for code in codes.tolist():
        ones.set(code, 1)
    assert 0 < want.sum() < _want(sb, rows, k, ones, 1, 2)[:, 1].sum() and want[:, 0].sum() > 0 and want[:, -1].sum() > 0


# 5 ---- crowded buckets: filled through the general merge (chains may run a whole bucket) to a load of 0.6 and more; half of the
# looked-up k-mers are absent, so probes wrap the bucket's end and absent k-mers end far from home
def test_crowded_buckets():
    k, log2_slots, log2_bucket = 21, 13, 10
    text_a, text_c = _text(_runs(500 + k)), _text(_runs(900 + k))
    # the text length with the oracle: read pairs (302 characters each) until the table holds 0.62 x 2^13 distinct k-mers
    otab, n_chars = oracle.Table(k), 0
    while len(otab) < 0.62 * (1 << log2_slots):
        otab.count(text_a[n_chars:n_chars + 302])
        n_chars += 302
    assert n_chars < len(text_a) and len(otab) <= 0.7 * (1 << log2_slots)
    src = kmer.count_kmers(_stream([("a", text_a[:n_chars])]), k, kind="hash")
    t = kmer.KmerTable.mini_with_slots(k, DEV, log2_slots, log2_bucket)
    t.add_table(src)
    # (occupied slots per bucket; ``bucket_fill()`` itself serves hash tables only)
    fill = (t.data.view(t.n_buckets, -1) != 0).sum(dim=1).cpu().numpy()
    assert fill.sum() == len(otab) and fill.sum() >= 0.6 * (1 << log2_slots) and fill.max() >= 0.6 * (1 << log2_bucket)
    # four rows: two of reads the table was counted from, two of another genome set
    b = (("h0", text_a[n_chars - 8 * 302:n_chars - 4 * 302]), ("c0", text_c[302:5 * 302]), ("h1", text_a[n_chars - 4 * 302:n_chars]), ("c1", text_c[5 * 302:9 * 302]))
    assert 0.25 <= _share(k, otab, _text(b)) <= 0.75
    sb = _stream(b)
    rows = sb.rows(302)
    assert len(rows) == 4
    assert np.array_equal(_rows(t, sb, kmer.Plan(rows, DEV)), _want(sb, rows, k, otab, 10, 400))


# 6 ---- rows that do not cover the stream (records outside every row), a row with runs of N
@pytest.mark.parametrize("k", [14, 21])
def test_rows_that_do_not_cover_the_stream(k):
    a, c = _runs(500 + k, 300, 20), _runs(900 + k, 300, 20)
    b = list(_second_half_plus(a, c))
    one = b[3][1]
    b.insert(4, ("holes", one[:40] + b"N" * 45 + one[85:400] + b"NNNN" + one[404:409] + b"N" + one[410:700] + b"N" * 64 + one[764:]))
    # runs too short to be rows: their records belong to no row
    for at, n in ((1, 120), (7, 299), (12, 31), (len(b), 250)):
        b.insert(at, (f"short{n}", one[700:700 + n] + b"N"))
    sb = _stream(b)
    rows = sb.rows(302)
    assert len(rows) == len(b) - 4 and "holes" in rows.names and not any(n.startswith("short") for n in rows.names)
    otab = _otable(k, _text(a))
    want = _want(sb, rows, k, otab, 10, 400)
    t = _mini(k, 20, 10, _stream(a))
    assert np.array_equal(_rows(t, sb, kmer.Plan(rows, DEV)), want)


# 7 ---- loaded and merged tables
def test_loaded_and_merged_tables(tmp_path):
    k = 21
    a, c = _runs(500 + k), _runs(900 + k)
    b = _second_half_plus(a, c)
    sa, sb, sc = _stream(a), _stream(b), _stream(c[:len(c) // 2])
    rows = sb.rows(302)
    plan = kmer.Plan(rows, DEV)
    ta = _mini(k, 20, 10, sa)
    want_a = _want(sb, rows, k, _otable(k, _text(a)), 10, 400)
    # write_dump -> from_dump
    path = str(tmp_path / "a.dump")
    ta.write_dump(path)
    loaded = kmer.KmerTable.from_dump(path, k, DEV, kind="mini")
    assert loaded.kind == "mini"
    assert np.array_equal(_rows(loaded, sb, plan), want_a)
    # the sum of two tables, bucket by bucket (one geometry) and through add_table (two geometries)
    want_ac = _want(sb, rows, k, _otable(k, _text(a), _text(c[:len(c) // 2])), 10, 400)
    assert not np.array_equal(want_ac, want_a)
    aligned = kmer.KmerTable.merged([ta, _mini(k, 20, 10, sc)])
    assert aligned.merge_form == "aligned" and aligned.kind == "mini"
    assert np.array_equal(_rows(aligned, sb, plan), want_ac)
    general = kmer.KmerTable.merged([ta, _mini(k, 18, 12, sc)])
    assert general.merge_form == "general" and general.kind == "mini"
    assert np.array_equal(_rows(general, sb, plan), want_ac)
    # the same table twice: every count doubled
    want_2a = _want(sb, rows, k, _otable(k, _text(a), _text(a)), 10, 400)
    assert np.array_equal(_rows(kmer.KmerTable.merged([ta, ta]), sb, plan), want_2a)


def test_a_given_hash_table_is_converted_once(tmp_path, monkeypatch, caplog):
    """compute_features(table = a hash table, 13 <= k <= 21) makes a mini table of it and takes the find form"""
    k = 15
    cfg = synth.SynthConfig(n_pairs=300, n_barcodes=7, n_genomes=3, genome_len=30_000, fragment=8_000, sub_rate=0.01, n_rate=0.2, seed=900 + k)
    fq = str(tmp_path / "c.fq")
    synth.write_fastq(synth.generate(cfg, device="cpu"), cfg, fq)
    s = ReadStream.from_fastq(fq, device=DEV)
    text = s.decode()
    otab = _otable(k, _text(_runs(500 + k)), text[:len(text) // 2])
    assert 0.25 <= _share(k, otab, text) <= 0.75
    h = kmer.KmerTable.from_items(k, *otab.items(), DEV, kind="hash")
    assert h.kind == "hash"
    seen = []
    real = kmer.KmerTable.abundance_of
    monkeypatch.setattr(kmer.KmerTable, "abundance_of", lambda self, *a, **kw: (seen.append(self), real(self, *a, **kw))[1])
    before = h.data.clone()
    with caplog.at_level("INFO"):
        names, _, abd = feature.compute_features(fq, None, k, 0, 10, 400, 302, device=torch.device(DEV), want_tnf=False, table=h)
    assert len(seen) == 1 and seen[0] is not h and seen[0].kind == "mini" and seen[0].rows_form == "find"
    assert any("mini table" in r.getMessage() for r in caplog.records)
    assert torch.equal(h.data, before)
    rows = s.rows(302)
    assert names == list(rows.names)
    assert np.array_equal(abd, _want(s, rows, k, otab, 10, 400))


# 8 ---- nothing is written where it should not be: the table by ``_rows``; every store of the new kernel by the checked build
def test_find_kernel_through_the_checked_build():
    """the same library built with -DPG_CHECKED (every global store of the super-k-mer kernels checks its index against the capacity
    of the buffer it writes into; PG_STATUS_BOUNDS instead of a memory fault): the oracle cases of this file run through it in a
    process of their own.  New kernel code is run this way first -- see DESIGN.md section 4, 'the abort'."""
    if os.environ.get("PANGAEA_LIB") == "checked":
        pytest.skip("already inside the checked pass")
    env = dict(os.environ, PANGAEA_LIB="checked")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_mini_find_gpu.py"),
                        "-k", "same_reads or other_reads or nothing_shared or chosen_counts or crowded or do_not_cover or loaded_and_merged"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# 9 ---- fallbacks: the lookup form, with the rows it always gave
def test_fallbacks_take_the_lookup_form(monkeypatch):
    a, c = _runs(521), _runs(921)
    b = _second_half_plus(a, c)
    sa, sb = _stream(a), _stream(b)
    rows = sb.rows(302)
    plan = kmer.Plan(rows, DEV)
    # a miniw table (22 <= k <= 31)
    w = kmer.KmerTable.mini_with_slots(25, DEV, 20, 13).count(sa)
    assert w.kind == "miniw"
    assert np.array_equal(_rows(w, sb, plan, form="lookup"), _want(sb, rows, 25, _otable(25, _text(a)), 10, 400))
    t = _mini(21, 20, 10, sa)
    otab = _otable(21, _text(a))
    # window x vsize beyond the packed counts' exact range: the lookup form, which refuses it as it always did
    t.rows_form = None
    with pytest.raises(_lib.PangaeaError, match="exceeds the exact range of the hash table"):
        t.abundance_of(sb, plan, SAT // 400 + 1, 400)
    assert t.rows_form == "lookup"
    with pytest.raises(_lib.PangaeaError, match="exceeds the exact range of the hash table"):
        kmer.features(sb, plan, k_tnf=None, table=t, window=SAT // 400 + 1, vsize=400)
    # a hash table
    h = kmer.count_kmers(sa, 21, kind="hash")
    want = _want(sb, rows, 21, otab, 10, 400)
    assert np.array_equal(_rows(h, sb, plan, form="lookup"), want)
    # PG_MINI_FIND=0, read at call time -- in abundance_of and in features()
    assert np.array_equal(_rows(t, sb, plan), want)
    monkeypatch.setenv("PG_MINI_FIND", "0")
    assert np.array_equal(_rows(t, sb, plan, form="lookup"), want)
    t.rows_form = None
    tnf0, abd0 = kmer.features(sb, plan, k_tnf=4, table=t, window=10, vsize=400)
    assert t.rows_form is None and np.array_equal(abd0.cpu().numpy(), want)
    monkeypatch.delenv("PG_MINI_FIND")
    tnf1, abd1 = kmer.features(sb, plan, k_tnf=4, table=t, window=10, vsize=400)
    assert t.rows_form == "find" and torch.equal(abd1, abd0) and torch.equal(tnf1, tnf0)
    # a stream that would be counted in pieces
    monkeypatch.setenv("PANGAEA_MINI_PIECE_WORDS", str(_lib.WORD_ALIGN))
    big = _mini(21, 22, 10, sa)
    assert np.array_equal(_rows(big, sb, plan, form="lookup"), want)


# 10 ---- one GPU, -1 / -2 input with qualities below '?': the table leaves those bases out, the rows do not
def test_quality_masked_pairs_take_the_find_form(tmp_path, monkeypatch):
    r1, r2 = os.path.join(GOLDEN, "pairq_R1.fq"), os.path.join(GOLDEN, "pairq_R2.fq")
    seen = []
    real = kmer.KmerTable.abundance_of
    monkeypatch.setattr(kmer.KmerTable, "abundance_of", lambda self, *a, **kw: (seen.append(self), real(self, *a, **kw))[1])
    got = {}
    for find in ("1", "0"):
        monkeypatch.setenv("PG_MINI_FIND", find)
        for k, w, v in ((15, 1, 6), (21, 1, 6)):
            got[find, k] = feature.compute_features(r1, r2, k, 4, w, v, 100, device=torch.device(DEV))
    assert len(seen) == 2 and all(t.kind == "mini" and t.rows_form == "find" for t in seen)
    s = ReadStream.from_fastq(r1, r2, device=DEV)
    assert s.valid_lowq is not None and not s.rows_inside_table
    rows = s.rows(100)
    for k in (15, 21):
        names, tnf, abd = got["1", k]
        names0, tnf0, abd0 = got["0", k]
        assert names == names0 and np.array_equal(tnf, tnf0) and np.array_equal(abd, abd0)
        otab = oracle.Table.from_dump(os.path.join(GOLDEN, f"pairq.k{k}.dump"), k)
        assert np.array_equal(abd, _want(s, rows, k, otab, 1, 6))
    # count_kmer -1 -2 -g DUMP
    out = {}
    for find in ("1", "0"):
        monkeypatch.setenv("PG_MINI_FIND", find)
        out[find] = str(tmp_path / f"abd{find}.csv.gz")
        assert cli.main_count_kmer(["-1", r1, "-2", r2, "-g", os.path.join(GOLDEN, "pairq.k15.dump"), "-k", "15", "-w", "1", "-v", "6", "-l", "100",
                                    "-o", out[find]]) == 0
    assert len(seen) == 3 and seen[2].kind == "mini" and seen[2].rows_form == "find"
    with gzip.open(out["1"], "rb") as f, gzip.open(out["0"], "rb") as g:
        text = f.read()
        assert len(text) > 0 and text == g.read()
