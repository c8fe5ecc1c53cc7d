#!/usr/bin/env python3
"""Writes tests/golden/fastq_rounds.json: what the two round rules said of every stub state BEFORE they became
``fastqtext.take_round`` -- ``kmer._filter_round`` (filter / trim / correct / normalize) and ``prepreads._round`` (preprocess).  To be
run at the commit in front of that change (54357d8), from the repository root:

    python tests/golden/make_round_goldens.py

The file: ``messages`` (every distinct pending message, once) and ``blocks``, one per (flavour, number of inputs): ``flavour`` is
"any", "both", "single" (``_filter_round``) or "prep" (``_round``), ``grid`` names the per-input states -- ``GRIDS`` below, shared with
the test -- and ``rows`` holds one row per stub state, in the order of ``itertools.product(grid, repeat=inputs)``:
[n, index into messages or -1 for none, all_eof as 0 / 1].  A per-input state (n_rec, extra, eof) is a piece with
``n_lines = 4 * n_rec + extra``, as ``_FastqPieces.index`` leaves it: before the end of the file a torn last line is not among the
lines, so every (n_rec, extra) of a grid exists under both values of ``eof``.  Every input has 6 records of earlier pieces behind
it (``done``: even, as an interleaved file under any / both leaves it)."""
import itertools
import json
import os
import sys
from types import SimpleNamespace

DONE = 6
PATHS = ("a.fq", "b.fq", "c.fq")
GRIDS = {"full": [(r, x, e) for r in range(4) for x in range(4) for e in (False, True)],
         "reduced": [(r, x, e) for r in range(3) for x in (0, 2) for e in (False, True)]}
BLOCKS = [(f, 1, "full") for f in ("any", "both", "single")] + [(f, 2, "full") for f in ("any", "both", "prep")] + [("prep", 3, "reduced")]


def stubs(states):
    return [SimpleNamespace(path=p, n_rec=r, n_lines=4 * r + x, eof=e, done=DONE) for p, (r, x, e) in zip(PATHS, states)]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from pangaea_amd.kmer import _filter_round
    from pangaea_amd.prepreads import _round
    messages, blocks = [], []
    for flavour, n_inputs, grid in BLOCKS:
        rows = []
        for states in itertools.product(GRIDS[grid], repeat=n_inputs):
            ins = stubs(states)
            n, pending, all_eof = _round(ins) if flavour == "prep" else _filter_round(ins, flavour != "single", flavour)
            if pending is not None and pending not in messages:
                messages.append(pending)
            rows.append([n, -1 if pending is None else messages.index(pending), int(all_eof)])
        blocks.append({"flavour": flavour, "inputs": n_inputs, "grid": grid, "rows": rows})
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_rounds.json")
    with open(out, "w") as f:
        dumps = lambda v: json.dumps(v, separators=(",", ":"))      # noqa: E731  (a message, a block per line)
        f.write('{"messages":[\n' + ",\n".join(map(dumps, messages)) + '\n],"blocks":[\n' + ",\n".join(map(dumps, blocks)) + "\n]}\n")
    print(out, os.path.getsize(out), "bytes,", len(messages), "messages,", sum(len(b["rows"]) for b in blocks), "rows")
