"""The second scatter pass of the super-k-mer pipeline (``mini_scatter2_kernel``) on both of its forms: 256 digits (tables of up to
2^15 buckets: 256 lanes x 16 records, about one tile per workgroup) and 512 digits (2^16 buckets: 512 lanes x 24 records per tile,
at most 16 workgroups per region that walk its tiles with the next one prefetched, the k-mer tally in counters of its own).

A bucket of a table with 2^16 buckets is half of a bucket of the same table with 2^15 (the bucket is the top bits of one product),
so the two forms must agree exactly: the records of buckets 2i and 2i + 1 are, as a multiset and class by class, the records of
bucket i; the k-mers-in-rows tally (``kwords``, the word-wise lookups' sizes) of 2i and 2i + 1 add up to that of i.  Checked on
streams whose regions hold a few records (less than one tile, most digits empty) and many tiles each, then tables and rows
against the key-partitioned kernels and the oracle."""
import numpy as np
import pytest
import torch

from oracle import oracle
from pangaea_amd import _lib, kmer, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHORT_MAX = 4                      # PG_SHORT_MAX: a record of at most this many k-mers is "short"


def _r256(x):
    return (x + 255) // 256 * 256


def _plan_planes(t):
    """off[nb + 1], cur2[nb] (short records per bucket), kwords[nb] of the plan workspace the last count used (the layout of
    plan_mini in mini.hip: header | region_tot | region_off | off | hist | cur2 | cur2l | kwords | ...)"""
    nb = t.n_buckets
    ws = t._mini_plan[1]
    o_off = 512 + _r256(256 * 8) + _r256(257 * 8)
    o_hist = o_off + _r256((nb + 1) * 8)
    o_cur2 = o_hist + _r256(nb * 8)
    o_kw = o_cur2 + 2 * _r256(nb * 8)
    q = lambda o, n: ws[o:o + 8 * n].view(torch.int64)
    return q(o_off, nb + 1).clone(), q(o_cur2, nb).clone(), q(o_kw, nb).clone()


def _bucket_records(t):
    """(bucket of the 2^15-bucket table, class, base, meta without its digit bits) of every record after the second pass, sorted"""
    off, cur2, _ = _plan_planes(t)
    nb = t.n_buckets
    n = int(off[nb])
    assert int(off[0]) == 0 and bool((off[1:] >= off[:-1]).all()) and n == t.plan_counts()[0]
    ws = t._mini_rec_ws
    cap = _lib.check(_lib.load().pg_mini_records_meta_offset(ws.numel(), t.desc())) // 20    # [bases A | bases B | meta A | meta B]
    bases = ws[8 * cap:16 * cap].view(torch.int64)[:n]
    meta = ws[20 * cap:24 * cap].view(torch.int32)[:n].to(torch.int64) & 0xffffffff
    b = torch.repeat_interleave(torch.arange(nb, device=ws.device), off[1:] - off[:-1])
    pos = torch.arange(n, device=ws.device)
    cls = (pos >= off[:-1][b] + cur2[b]).to(torch.int64)                 # short records at the front of their bucket, long at the back
    bits2 = (nb.bit_length() - 1) - 8
    assert bool(((meta & ((1 << bits2) - 1)) == (b & ((1 << bits2) - 1))).all()), "a record outside its bucket"
    length = ((meta >> 8) & 15) + 1
    assert bool(((length > SHORT_MAX).to(torch.int64) == cls).all()), "a record in the other class"
    b15 = b >> (nb.bit_length() - 1 - 15)
    key = (b15 << 41) | (cls << 40) | (meta >> 8)
    order = torch.sort(bases, stable=True).indices
    order = order[torch.sort(key[order], stable=True).indices]
    return torch.stack([key[order], bases[order]])


@pytest.mark.parametrize("n_pairs,n_genomes,genome_len,sub_rate", [
    (1_500, 2, 20_000, 0.01),        # a few records per region: less than one tile, most of the 512 digits empty
    (1_200_000, 4, 150_000, 0.0),    # ~23 tiles of 12 288 records per region: workgroups of the 512-digit form walk one or two
])
def test_both_second_pass_forms_put_the_same_records_into_the_same_buckets(n_pairs, n_genomes, genome_len, sub_rate, monkeypatch):
    cfg = synth.SynthConfig(n_pairs=n_pairs, n_barcodes=max(1, n_pairs // 200), n_genomes=n_genomes, genome_len=genome_len,
                            fragment=8_000, sub_rate=sub_rate, n_rate=0.01, seed=77)
    s = synth.generate(cfg, device=DEV)
    rows = s.rows(1000)
    plan = kmer.Plan(rows, DEV)
    got = {}
    for merged in (False, True):
        for lb in (9, 8):                                               # 2^24 slots: 2^15 buckets (256 digits), 2^16 (512 digits)
            monkeypatch.setenv("PG_MINI_MERGE", "1" if merged else "0")
            t = kmer.KmerTable.mini_with_slots(21, DEV, 24, lb).count(s, rows=plan, emit=(10, 400))
            assert t.n_buckets == 1 << (24 - lb)
            recs = _bucket_records(t)
            _, _, kw = _plan_planes(t)
            _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=10, vsize=400)
            got[(lb, merged)] = (t.items(), abd, recs, kw)
            del t
    monkeypatch.delenv("PG_MINI_MERGE", raising=False)
    (codes, counts), abd, recs, kw15 = got[(9, False)]
    assert int(recs.shape[1]) > 0 and int(kw15.sum()) > 0
    for key, (items, a, r, kw) in got.items():
        assert np.array_equal(items[0], codes) and np.array_equal(items[1], counts), key
        assert torch.equal(a, abd), key
        assert torch.equal(r, recs), key
    # the word-wise form's tally: 2^16-bucket pairs add up to the 2^15-bucket one (the merged form does not keep one)
    kw16 = got[(8, False)][3]
    assert torch.equal(kw16.view(-1, 2).sum(1), kw15)
    # the key-partitioned kernels count the same table and rows
    other = kmer.count_kmers(s, 21, kind="hash", rows=plan, emit=(10, 400))
    o_items = other.items()
    assert np.array_equal(o_items[0], codes) and np.array_equal(o_items[1], counts)
    _, abd_o = kmer.features(s, plan, k_tnf=None, table=other, window=10, vsize=400)
    assert torch.equal(abd_o, abd)
    if n_pairs <= 10_000:
        text = s.decode()
        otab = oracle.Table(21, threads=4).count(text)
        assert len(otab) == len(codes)
        for r in range(len(rows)):
            assert np.array_equal(abd[r].cpu().numpy(), oracle.abd_row(text[rows.start[r]:rows.end[r]], 21, otab, 10, 400)), r


def test_one_gpu_default_geometry_and_the_a_b_switch(monkeypatch):
    """2^29-slot packed tables default to 2^16 buckets of 2^13 slots; PG_MINI_LOG2_BUCKET=14 gives 2^15 x 2^14 back; both count
    the same table and rows (the two-workgroups-per-CU count and the 512-digit second pass against the 1024-thread count and the
    256-digit one)"""
    monkeypatch.delenv("PG_MINI_LOG2_BUCKET", raising=False)
    cfg = synth.SynthConfig(n_pairs=20_000, n_barcodes=100, n_genomes=3, genome_len=60_000, fragment=8_000, sub_rate=0.01, seed=31)
    s = synth.generate(cfg, device=DEV)
    plan = kmer.Plan(s.rows(1000), DEV)
    res = {}
    for want in (None, "14"):
        if want:
            monkeypatch.setenv("PG_MINI_LOG2_BUCKET", want)
        t = kmer.KmerTable.mini_with_slots(21, DEV, 29).count(s, rows=plan, emit=(10, 400))
        _, abd = kmer.features(s, plan, k_tnf=None, table=t, window=10, vsize=400)
        res[want] = (t.log2_bucket, t.n_buckets, t.items(), abd)
        del t
        torch.cuda.empty_cache()
    assert res[None][:2] == (13, 1 << 16) and res["14"][:2] == (14, 1 << 15)
    (c0, n0), (c1, n1) = res[None][2], res["14"][2]
    assert np.array_equal(c0, c1) and np.array_equal(n0, n1)
    assert torch.equal(res[None][3], res["14"][3])
