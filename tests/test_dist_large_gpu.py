"""The N-rank super-k-mer form at the size of a real share (10 M read pairs, 50 000 rows), in a one-rank RCCL group on cuda:0.
Below about 1 GB the exchange's all-to-all arrived whole; the entries of a 10 M-pair share (1.39 GB) in ONE RCCL call arrived
only half, and the rows of dist.MiniSharded then differed from the one-GPU rows on nearly every row, plain input included."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from pangaea_amd import dist as pdist
from pangaea_amd import kmer, synth

K, W, V = 21, 10, 400


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rccl(fn, *args):
    mp.spawn(fn, args=(_free_port(),) + args, nprocs=1, join=True)


def _init(port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))


def _a2a_worker(rank, port):
    _init(port)
    try:
        inp = torch.arange(200_000_000, dtype=torch.int64, device="cuda:0")            # 1.6 GB
        out = torch.zeros_like(inp)
        pdist._all_to_all_flat(out, inp)
        torch.cuda.synchronize()
        assert torch.equal(out, inp)
        b = torch.arange(1 << 20, dtype=torch.int64, device="cuda:0").to(torch.int16)     # (a small one: one call, as before)
        ob = torch.zeros_like(b)
        pdist._all_to_all_flat(ob.view(torch.uint8), b.view(torch.uint8))
        assert torch.equal(ob, b)
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_the_exchange_all_to_all_delivers_a_large_buffer_whole():
    _rccl(_a2a_worker)


def _share_worker(rank, port, mask):
    _init(port)
    try:
        dev = torch.device("cuda", 0)
        s = synth.generate(synth.SynthConfig(n_pairs=10_000_000, n_barcodes=50_000, read_len=150, seed=2022), device=dev,
                           chunk_pairs=1 << 17, with_names=False)
        lc = False
        if mask == "qual":                                   # about 7 % of the bases below the quality threshold
            g = torch.Generator(device=dev)
            g.manual_seed(5)
            bits = (torch.rand((s.n_words, 32), device=dev, generator=g) < 0.07).to(torch.int64) << torch.arange(32, device=dev)
            q = bits.sum(dim=1)
            s.valid_lowq = torch.where(q >= (1 << 31), q - (1 << 32), q).to(torch.int32) & s.valid
        plan = kmer.Plan(s.rows(2000), dev)
        assert plan.n_rows == 50_000
        regs = kmer.distinct_sketch(s, K)
        local = kmer.sketch_estimate(kmer.distinct_sketch(s, K, plane=s.union_valid(lc)))
        log2_u, lb_u, lb_l = pdist.MiniSharded.geometry(max(1 << 14, int(1.05 * kmer.sketch_estimate(regs))), int(1.1 * local), n_rows=plan.n_rows)
        ms = pdist.MiniSharded(K, dev, log2_u, lb_l, W, V, union_log2_bucket=lb_u, masked=mask != "none")
        ms.count(s, plan)
        assert ms.bytes_sent == 0 and ms._cap1 * 8 > (1 << 30)          # (one rank: a buffer past the size that arrived whole in one call)
        _, abd = kmer.features(s, plan, k_tnf=None, table=ms.local, window=W, vsize=V)
        n_union = int((ms.union.data != 0).sum())
        del ms
        torch.cuda.empty_cache()
        one = kmer.count_kmers(s, K, rows=plan, emit=(W, V))
        _, want = kmer.features(s, plan, k_tnf=None, table=one, window=W, vsize=V)
        assert int((abd != want).any(dim=1).sum()) == 0
        assert n_union == int((one.data != 0).sum())
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("mask", ["none", "qual"])
def test_a_10m_pair_share_gives_the_one_gpu_rows(mask):
    _rccl(_share_worker, mask)
