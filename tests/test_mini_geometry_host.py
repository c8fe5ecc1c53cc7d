"""CPU-only checks of the default bucket size of super-k-mer tables (``KmerTable.mini_default_log2_bucket``): packed tables of
2^29 slots and more take 2^16 buckets of 2^13 slots, everything else keeps the largest bucket LDS holds; the constant is the
header's."""
import os
import re

import pytest

from pangaea_amd import _lib, kmer


def test_the_constant_is_the_headers():
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "pangaea_feat.h")).read()
    m = re.search(r"#define PG_MINI_LARGE_LOG2_BUCKET_SLOTS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MINI_LARGE_LOG2_BUCKET_SLOTS


@pytest.mark.parametrize("k,log2_slots,want", [
    (21, 29, 13),      # the one-GPU bench table: 2^16 x 2^13 (until round 5: 2^15 x 2^14)
    (21, 30, 14),      # 2^16 buckets of the largest size
    (21, 28, 14),      # smaller tables: unchanged
    (21, 20, 14),
    (21, 12, 12),      # one bucket
    (15, 29, 13),
    (13, 29, 13),
    (22, 29, 13),      # 12-byte slots: 2^13 is already the largest bucket
    (31, 28, 13),
])
def test_default_bucket(k, log2_slots, want):
    assert kmer.KmerTable.mini_default_log2_bucket(k, log2_slots) == want
    assert kmer.KmerTable.mini_applies(k, log2_slots, want)

