"""``fastqtext.line_index`` as a function of the text alone (pg_fastq_index): line starts and line counts compared exactly with
``numpy.flatnonzero`` on the host, on texts of more lines than the first capacity ``n_bytes // 16 + 1024`` holds, so that the
index is asked for a second time with room; the buffers a ``hold`` keeps; and a text that is a view at an odd offset."""
import numpy as np
import pytest
import torch

from pangaea_amd import fastqtext, kmer, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def want_index(data: bytes) -> np.ndarray:
    """line_start[j] for j < lines, then n_bytes (include/pangaea_feat.h, pg_fastq_index): a last line without '\\n' is a line"""
    a = np.frombuffer(data, np.uint8)
    starts = np.concatenate([[0], np.flatnonzero(a == 10) + 1])
    return starts if data.endswith(b"\n") else np.concatenate([starts, [len(data)]])


TEXTS = {"4096-one-byte-lines": b"A\n" * 4096, "no-final-newline": (b"A\n" * 4096)[:-1], "empty-lines": b"\n" * 3000}


@pytest.mark.parametrize("name", list(TEXTS))
def test_line_index_of_more_lines_than_the_first_capacity(name):
    data = TEXTS[name]
    want = want_index(data)
    assert len(want) > len(data) // 16 + 1024                # (the first call cannot hold them: the second one is what is tested)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
    hold = {}
    idx, n_lines = fastqtext.line_index(text, len(data), hold)
    assert n_lines == len(want) - 1 and idx.dtype == torch.int64 and idx.device == text.device
    assert np.array_equal(idx[:n_lines + 1].cpu().numpy(), want)
    # the same hold again: the buffers it kept serve the second call, which needs no second ask
    kept = idx.data_ptr(), hold["idx"].data_ptr(), hold["ws"].data_ptr()
    idx2, n_lines2 = fastqtext.line_index(text, len(data), hold)
    assert (idx2.data_ptr(), hold["idx"].data_ptr(), hold["ws"].data_ptr()) == kept and n_lines2 == n_lines
    assert np.array_equal(idx2[:n_lines + 1].cpu().numpy(), want)
    # without a hold: buffers of its own
    idx3, n_lines3 = fastqtext.line_index(text, len(data))
    assert n_lines3 == n_lines and idx3.data_ptr() != kept[0] and torch.equal(idx3[:n_lines + 1], idx[:n_lines + 1])


def test_a_view_at_an_odd_offset_reads_as_its_clone():
    reads = synth.generate(synth.SynthConfig(n_pairs=40, n_barcodes=2, n_genomes=2, genome_len=20_000, fragment=8_000, seed=11), device=DEV)
    table = kmer.KmerTable.alloc(4, DEV, "dense").count(reads)
    seqs = reads.decode().split(b"N")[:9]
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    text = torch.frombuffer(bytearray(b"xyz" + data), dtype=torch.uint8).to(DEV)[3:]
    assert text.data_ptr() & 15
    got, want = table.read_hits(text), table.read_hits(text.clone())
    assert got.shape == (len(seqs), 2) and int(got[:, 0].sum()) > 0 and torch.equal(got, want)
    assert np.array_equal(fastqtext.line_index(text.clone(), len(data))[0][:4 * len(seqs) + 1].cpu().numpy(), want_index(data))
