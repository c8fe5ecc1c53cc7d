"""What the super-k-mer entry points of the library refuse, and in which words: every call here carries a descriptor whose
addresses are fake (non-null, never dereferenced) and one argument that the entry point turns down BEFORE it touches the GPU --
so the return code and the exact pg_last_error() text are checked on the host.  No kernel is launched, no HIP call is made."""
import ctypes as C

import pytest

from pangaea_amd import _lib

EINVAL = -1
FAKE = 0x7F0000000000            # a 256-byte aligned address that belongs to nobody
ODD = FAKE + 8                   # ... and one that is not aligned
HUGE = 1 << 45                   # bytes of a workspace that is certainly large enough
N_WORDS, WINDOW, VSIZE = 8192, 10, 400


def _table(kind=_lib.TABLE_MINI, k=21, log2_slots=20, log2_bucket_slots=10, data=FAKE):
    return _lib.pg_table(kind, k, log2_slots, log2_bucket_slots, data)


MINI = _table()                                                     # 2^10 buckets of 2^10 slots
WIDE = _table(kind=_lib.TABLE_MINI_WIDE, k=25)                      # the same geometry, 8-byte keys + counts
FEW = _table(log2_slots=18)                                         # 2^8 buckets: no second scatter pass


def _rows(n=1000):
    return _lib.pg_rows(FAKE, FAKE, n, None)


ROWS = _rows()


def _sizes(t):
    L = _lib.load()
    return L.pg_mini_plan_bytes(N_WORDS, C.byref(t)), L.pg_mini_records_bytes(50_000, C.byref(t)), L.pg_mini_half_bytes(C.byref(t))


# ---- the argument lists of the entry points, all acceptable; a case replaces some of them by name
def _plan(**kw):
    a = dict(codes=FAKE, valid=FAKE, word_begin=0, word_end=N_WORDS, t=MINI, rows=ROWS, plan_ws=FAKE, plan_ws_bytes=HUGE, stream=None)
    return "pg_mini_plan", a, kw


def _plan_masked(**kw):
    a = dict(codes=FAKE, valid=FAKE, table_valid=FAKE, word_begin=0, word_end=N_WORDS, t=MINI, rows=ROWS, plan_ws=FAKE, plan_ws_bytes=HUGE, stream=None)
    return "pg_mini_plan_masked", a, kw


_COUNT = dict(codes=FAKE, valid=FAKE, word_begin=0, word_end=N_WORDS, t=MINI, rows=ROWS, plan_ws=FAKE, plan_ws_bytes=HUGE, rec_ws=FAKE, rec_ws_bytes=HUGE,
              window=WINDOW, vsize=VSIZE)


def _count(**kw):
    a = dict(_COUNT, shuffle_ws=FAKE, shuffle_ws_bytes=HUGE, merge_ws=FAKE, merge_ws_words=1 << 30, status=FAKE, stream=None)
    return "pg_mini_count", a, kw


def _count_piece(**kw):
    a = dict(_COUNT, merge_ws=FAKE, merge_ws_words=1 << 30, first=1, status=FAKE, stream=None)
    return "pg_mini_count_piece", a, kw


def _count_half(masked=False, **kw):
    a = dict(_COUNT, shuffle_ws=FAKE, shuffle_ws_bytes=HUGE, merge_ws=FAKE, merge_ws_words=1 << 30, half_ws=FAKE, half_ws_bytes=HUGE, fill=FAKE,
             status=FAKE, stream=None)
    if masked:
        a = dict(codes=a.pop("codes"), valid=a.pop("valid"), table_valid=FAKE, **a)
    return "pg_mini_count_half_masked" if masked else "pg_mini_count_half", a, kw


def _count_half_piece(masked=False, **kw):
    a = dict(_COUNT, merge_ws=FAKE, merge_ws_words=1 << 30, half_ws=FAKE, half_ws_bytes=HUGE, fill=FAKE, first=1, last=0, status=FAKE, stream=None)
    if masked:
        a = dict(codes=a.pop("codes"), valid=a.pop("valid"), table_valid=FAKE, **a)
    return "pg_mini_count_half_piece_masked" if masked else "pg_mini_count_half_piece", a, kw


def _lookup_piece(**kw):
    a = dict(t=MINI, rows=ROWS, plan_ws=FAKE, plan_ws_bytes=HUGE, n_words_piece=N_WORDS, meta=FAKE, n_words_total=4 * N_WORDS, window=WINDOW, vsize=VSIZE,
             shuffle_ws=FAKE, shuffle_ws_bytes=HUGE, merge_ws=FAKE, status=FAKE, stream=None)
    return "pg_mini_lookup_piece", a, kw


def _lookup_half(**kw):
    a = dict(t=MINI, rows=ROWS, plan_ws=FAKE, plan_ws_bytes=HUGE, rec_ws=FAKE, rec_ws_bytes=HUGE, n_words_counted=N_WORDS, vsize=VSIZE, shuffle_ws=FAKE,
             shuffle_ws_bytes=HUGE, merge_ws=FAKE, merge_ws_words=1 << 30, half_ws=FAKE, half_ws_bytes=HUGE, bins_in=FAKE, bin_elem=FAKE, status=FAKE, stream=None)
    return "pg_mini_lookup_half", a, kw


def _lookup_half_piece(**kw):
    a = dict(t=MINI, rows=ROWS, plan_ws=FAKE, plan_ws_bytes=HUGE, n_words_piece=N_WORDS, meta=FAKE, n_words_total=4 * N_WORDS, vsize=VSIZE, shuffle_ws=FAKE,
             shuffle_ws_bytes=HUGE, merge_ws=FAKE, half_ws=FAKE, half_ws_bytes=HUGE, bins_in=FAKE, bin_elem=FAKE, status=FAKE, stream=None)
    return "pg_mini_lookup_half_piece", a, kw


def _gather(**kw):
    a = dict(t=MINI, half_ws=FAKE, half_ws_bytes=HUGE, fill=FAKE, dst_elem=FAKE, out=FAKE, out_elems=1000, status=FAKE, stream=None)
    return "pg_mini_gather_entries", a, kw


def _from_emitted(**kw):
    a = dict(t=MINI, rows=ROWS, vsize=VSIZE, abd_out=FAKE, plan_ws=FAKE, plan_ws_bytes=HUGE, n_words_counted=N_WORDS, shuffle_ws=FAKE, shuffle_ws_bytes=HUGE,
             stream=None)
    return "pg_mini_abundance_from_emitted", a, kw


def _refused(call, text):
    name, args, kw = call
    unknown = set(kw) - set(args)
    assert not unknown, unknown
    args = dict(args, **kw)
    L = _lib.load()
    keep = [v for v in args.values() if isinstance(v, C.Structure)]               # (alive for the call)
    rc = getattr(L, name)(*[C.byref(v) if isinstance(v, C.Structure) else v for v in args.values()])
    del keep
    assert rc == EINVAL, (rc, L.pg_last_error())
    assert L.pg_last_error().decode() == text


def _cases():
    """(id, call, text) of the refusals that come before any HIP call in every version of the library"""
    plan_b, _, half_b = _sizes(MINI)
    return [
        # null pointers
        ("plan-null", _plan(codes=None), "pg_mini_plan: null argument"),
        ("plan_masked-null", _plan_masked(plan_ws=None), "pg_mini_plan: null argument"),
        ("plan-null-table", _plan(t=_table(data=None)), "pg_mini_plan: table descriptor is null"),
        ("plan-null-rows", _plan(rows=_lib.pg_rows(None, FAKE, 10, None)), "pg_mini_plan: null row arrays"),
        ("count-null", _count(status=None), "pg_mini_count: null argument"),
        ("count-null-shuffle", _count(shuffle_ws=None), "pg_mini_count: null shuffle workspace"),
        ("count-no-rows", _count(rows=None), "pg_mini_count: the lookup pass needs rows"),
        ("count_half-null", _count_half(fill=None), "pg_mini_count_half: null argument"),
        ("count_half_masked-null", _count_half(masked=True, half_ws=None), "pg_mini_count_half: null argument"),
        ("count_half_piece-null", _count_half_piece(half_ws=None), "pg_mini_count_half_piece: null argument"),
        ("lookup_piece-null", _lookup_piece(meta=None), "pg_mini_lookup_piece: bad argument"),
        ("lookup_half-null", _lookup_half(bins_in=None), "pg_mini_lookup_half: null argument"),
        ("lookup_half_piece-null", _lookup_half_piece(bin_elem=None), "pg_mini_lookup_half_piece: bad argument"),
        ("gather-null", _gather(out=None), "pg_mini_gather_entries: null argument"),
        ("from_emitted-null", _from_emitted(abd_out=None), "pg_mini_abundance_from_emitted: null argument"),
        # bad word range
        ("plan-range", _plan(word_begin=5, word_end=3), "pg_mini_plan: bad word range"),
        ("count-range", _count(word_begin=-1), "pg_mini_count: bad word range"),
        ("count_half_piece-range", _count_half_piece(word_begin=9, word_end=8), "pg_mini_count: bad word range"),
        # window / vsize
        ("count-window-alone", _count(vsize=0), "pg_mini_count: window 10 / vector size 0"),
        ("count-vsize-alone", _count(window=0), "pg_mini_count: window 0 / vector size 400"),
        ("count-vsize-large", _count(vsize=513), "pg_mini_count: window 10 x vector size 513 outside the exact range of the table"),
        ("count_piece-no-window", _count_piece(window=0, vsize=0), "pg_mini_count_piece: needs the abundance parameters and the slot buffer"),
        # plan workspace
        ("plan-small", _plan(plan_ws_bytes=plan_b - 256), f"pg_mini_plan: workspace of {plan_b - 256} bytes, {plan_b} needed"),
        ("plan-odd", _plan(plan_ws=ODD), "pg_mini_plan: workspace must be 256-byte aligned"),
        ("count-plan-small", _count(plan_ws_bytes=plan_b - 1), f"pg_mini_count: plan workspace of {plan_b - 1} bytes, {plan_b} needed"),
        ("count-plan-odd", _count(plan_ws=ODD), "pg_mini_count: workspaces must be 256-byte aligned"),
        ("count_half-plan-small", _count_half(plan_ws_bytes=0), f"pg_mini_count: plan workspace of 0 bytes, {plan_b} needed"),
        ("lookup_piece-plan-small", _lookup_piece(plan_ws_bytes=plan_b - 256), "pg_mini_lookup_piece: plan workspace does not match n_words_piece"),
        ("lookup_half-plan-small", _lookup_half(plan_ws_bytes=plan_b - 256), "pg_mini_lookup_half: plan workspace does not match n_words_counted"),
        ("lookup_half_piece-plan-small", _lookup_half_piece(plan_ws_bytes=plan_b - 256), "pg_mini_lookup_half_piece: plan workspace does not match n_words_piece"),
        ("from_emitted-plan-small", _from_emitted(plan_ws_bytes=plan_b - 256), "pg_mini_abundance_from_emitted: plan workspace does not match n_words_counted"),
        ("from_emitted-odd", _from_emitted(shuffle_ws=ODD), "pg_mini_abundance_from_emitted: workspace must be 256-byte aligned"),
        # record workspace
        ("count-rec-odd", _count(rec_ws=ODD), "pg_mini_count: workspaces must be 256-byte aligned"),
        ("count-rec-small", _count(rec_ws_bytes=24 * 256 - 1), "pg_mini_count: record workspace of 6143 bytes (pg_mini_records_bytes)"),
        ("count_piece-rec-small", _count_piece(rec_ws_bytes=0), "pg_mini_count: record workspace of 0 bytes (pg_mini_records_bytes)"),
        # half workspace
        ("count_half-half-small", _count_half(half_ws_bytes=half_b - 256), f"pg_mini_count_half: workspace of {half_b - 256} bytes (256-byte aligned), {half_b} needed"),
        ("count_half-half-odd", _count_half(half_ws=ODD, half_ws_bytes=half_b), f"pg_mini_count_half: workspace of {half_b} bytes (256-byte aligned), {half_b} needed"),
        ("count_half_masked-half-small", _count_half(masked=True, half_ws_bytes=1),
         f"pg_mini_count_half: workspace of 1 bytes (256-byte aligned), {half_b} needed"),
        ("count_half_piece-half-small", _count_half_piece(half_ws_bytes=half_b - 256),
         f"pg_mini_count_half_piece: workspace of {half_b - 256} bytes (256-byte aligned), {half_b} needed"),
        ("count_half_piece_masked-half-odd", _count_half_piece(masked=True, half_ws=ODD, half_ws_bytes=half_b),
         f"pg_mini_count_half_piece: workspace of {half_b} bytes (256-byte aligned), {half_b} needed"),
        ("lookup_half-half-small", _lookup_half(half_ws_bytes=half_b - 256), "pg_mini_lookup_half: workspace does not match the table"),
        ("lookup_half_piece-half-small", _lookup_half_piece(half_ws_bytes=half_b - 256), "pg_mini_lookup_half_piece: workspace does not match the table"),
        ("gather-half-small", _gather(half_ws_bytes=half_b - 256), "pg_mini_gather_entries: workspace does not match the table"),
        # a wide table given to a _piece or _half entry
        ("count_piece-wide", _count_piece(t=WIDE), "pg_mini_count_piece: packed mini tables (13 <= k <= 21)"),
        ("count_half_piece-wide", _count_half_piece(t=WIDE), "pg_mini_count_half_piece: packed mini tables (13 <= k <= 21)"),
        ("lookup_piece-wide", _lookup_piece(t=WIDE), "pg_mini_lookup_piece: bad argument"),
        ("lookup_half-wide", _lookup_half(t=WIDE), "pg_mini_lookup_half: not the slot form"),
        ("lookup_half_piece-wide", _lookup_half_piece(t=WIDE), "pg_mini_lookup_half_piece: bad argument"),
        # at most 256 buckets given to a lookup half
        ("lookup_piece-few", _lookup_piece(t=FEW), "pg_mini_lookup_piece: needs more than 256 buckets"),
        ("lookup_half-few", _lookup_half(t=FEW), "pg_mini_lookup_half: needs more than 256 buckets"),
        ("lookup_half_piece-few", _lookup_half_piece(t=FEW), "pg_mini_lookup_half_piece: needs more than 256 buckets"),
        # a piece without a slot buffer
        ("count_piece-no-buffer", _count_piece(merge_ws=None), "pg_mini_count_piece: needs the abundance parameters and the slot buffer"),
        ("count_half_piece-no-buffer", _count_half_piece(merge_ws_words=0), "pg_mini_count_half_piece: needs the abundance parameters and the slot buffer"),
        # rows the merged lookups do not apply to
        ("lookup_piece-rows", _lookup_piece(rows=_rows(1 << 20)), "pg_mini_lookup_piece: 1048576 rows (at most 1048574 per launch)"),
        ("lookup_half_piece-vsize", _lookup_half_piece(vsize=0), "pg_mini_lookup_half_piece: bad argument"),
    ]


def _late_cases():
    """refusals that used to come after the first launches (the count was enqueued, then the call failed): they now come before
    anything is enqueued, with the code and the text they always had"""
    L = _lib.load()
    shuf_b = L.pg_mini_shuffle_bytes_merged(N_WORDS, ROWS.n_rows, VSIZE, C.byref(MINI))
    return [
        ("count-merge-odd", _count(merge_ws=ODD), "pg_mini_count: workspaces must be 256-byte aligned"),
        ("count-shuffle-small", _count(shuffle_ws_bytes=shuf_b - 256),
         f"pg_mini_count: shuffle workspace of {shuf_b - 256} bytes (256-byte aligned), {shuf_b} needed"),
        ("count-shuffle-odd", _count(shuffle_ws=ODD, shuffle_ws_bytes=shuf_b), f"pg_mini_count: shuffle workspace of {shuf_b} bytes (256-byte aligned), {shuf_b} needed"),
        ("count_half-wide", _count_half(t=WIDE), "pg_mini_count_half: needs packed slots (k <= 21), rows and fewer than 2^(32 - log2 bucket slots) of them"),
        ("count_half-no-window", _count_half(window=0, vsize=0),
         "pg_mini_count_half: needs packed slots (k <= 21), rows and fewer than 2^(32 - log2 bucket slots) of them"),
        ("count_half-few", _count_half(t=FEW), "pg_mini_count_half: needs more than 256 buckets"),
        ("count_half_piece-few", _count_half_piece(t=FEW), "pg_mini_count_half: needs more than 256 buckets"),
        ("count_piece-no-words", _count_piece(merge_ws_words=0), "pg_mini_count_piece: needs the merged lookups (fewer than 2^20 rows, their slot buffer given)"),
        ("count_piece-rows", _count_piece(rows=_rows((1 << 20) - 2)), "pg_mini_count_piece: needs the merged lookups (fewer than 2^20 rows, their slot buffer given)"),
        ("count_half_masked-rows", _count_half(masked=True, rows=_rows(_lib.MINI_MASKED_MAX_ROWS + 1)),
         "pg_mini_count_half_masked: needs the merged lookups (their slot buffer given) and at most 524286 rows"),
        ("count_half_masked-no-buffer", _count_half(masked=True, merge_ws=None, merge_ws_words=0),
         "pg_mini_count_half_masked: needs the merged lookups (their slot buffer given) and at most 524286 rows"),
        ("count_half_piece_masked-rows", _count_half_piece(masked=True, rows=_rows(_lib.MINI_MASKED_MAX_ROWS + 1)),
         "pg_mini_count_half_masked: needs the merged lookups (their slot buffer given) and at most 524286 rows"),
        ("lookup_half-no-records", _lookup_half(rec_ws=None), "pg_mini_lookup_half: the merged form needs the count half's record workspace"),
        ("lookup_half-rec-small", _lookup_half(rec_ws_bytes=100), "pg_mini_lookup_half: record workspace of 100 bytes (pg_mini_records_bytes)"),
    ]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_refused_before_any_launch(case):
    _refused(case[1], case[2])


@pytest.mark.parametrize("case", _late_cases(), ids=lambda c: c[0])
def test_refused_before_anything_is_enqueued(case):
    _refused(case[1], case[2])


def test_record_workspace_layout_is_what_callers_are_told():
    """[bases A | bases B | meta A | meta B]: the second meta plane starts 20 bytes x capacity in, capacity = the largest
    multiple of 256 records that fits"""
    L = _lib.load()
    for n in (0, 1, 255, 256, 1000, 50_000):
        b = L.pg_mini_records_bytes(n, C.byref(MINI))
        cap = (n + 255) // 256 * 256 + 256
        assert b == 24 * cap
        for extra in (0, 1, 24 * 256 - 1):
            assert L.pg_mini_records_meta_offset(b + extra, C.byref(MINI)) == 20 * cap
    assert L.pg_mini_records_meta_offset(24 * 256 - 1, C.byref(MINI)) == EINVAL
    assert L.pg_last_error().decode() == "pg_mini_records_meta_offset: record workspace of 6143 bytes (pg_mini_records_bytes)"
