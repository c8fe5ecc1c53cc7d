"""``fastqtext.take_round`` against what the two round rules it replaced said of every stub state: tests/golden/fastq_rounds.json,
written by tests/golden/make_round_goldens.py (which says how to read it) at the commit in front of the change
(``kmer._filter_round``, ``prepreads._round``).  No GPU, no library: the rule reads ``n_rec``, ``n_lines``, ``eof``, ``done`` and
``path`` of its inputs and nothing else."""
import itertools
import json
import os

from pangaea_amd.fastqtext import take_round

from .golden.make_round_goldens import BLOCKS, GRIDS, stubs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fastq_rounds.json")


def pair_of(flavour):
    return None if flavour == "prep" else flavour


def test_every_state_of_the_grid_as_before():
    with open(GOLDEN) as f:
        golden = json.load(f)
    messages = golden["messages"]
    # one input under any / both / single, two under any / both / prep (the full grid of 32 states per input), three under prep (12)
    assert [(b["flavour"], b["inputs"], b["grid"]) for b in golden["blocks"]] == BLOCKS
    assert len(GRIDS["full"]) == 32 and len(GRIDS["reduced"]) == 12
    assert sum(len(b["rows"]) for b in golden["blocks"]) == 3 * 32 + 3 * 32 * 32 + 12 ** 3
    for b in golden["blocks"]:
        states = list(itertools.product(GRIDS[b["grid"]], repeat=b["inputs"]))
        assert len(states) == len(b["rows"])
        for st, (n, m, all_eof) in zip(states, b["rows"]):
            want = (n, None if m < 0 else messages[m], bool(all_eof))
            assert take_round(stubs(st), pair_of(b["flavour"])) == want, (b["flavour"], st)


def test_clean_end_beside_a_torn_end_keeps_both_answers():
    """input A ends cleanly at record n while input B ends INSIDE record n: the table verbs name the count mismatch, preprocess
    names the torn record"""
    states = [(2, 0, True), (2, 3, True)]
    uneven = "a.fq ends after 8 records, b.fq holds more: R1 and R2 must have the same number of records (PG_EFORMAT)"
    torn = "b.fq: record 8: the file ends inside it (3 of its 4 lines) (PG_EFORMAT)"
    for pair in ("any", "both"):
        assert take_round(stubs(states), pair) == (2, uneven, True)
    assert take_round(stubs(states), None) == (2, torn, True)
    # (preprocess names the mismatch in its own words where no record is torn)
    assert take_round(stubs([(2, 0, True), (3, 0, True)]), None)[1] == \
        "a.fq ends after 8 records, b.fq holds more: the read files must have the same number of records (PG_EFORMAT)"
