"""Option gcn_bf16_wide where there is no GPU: the mirror of its dispatch rule (tests/bf16_wide_ref.py, on aggregate_ref.dispatch)
against the built kernels, and the proof that the aggregations tests/test_gpu_bf16_wide_gather.py runs reach every instantiated wide
form -- 2, 3, 4 and 5 rows per lane group, loader wave on and off, one launch and two, pieces of split rows and hundreds of them,
several sweeps per slab, N = 8 -- and every fall-back: rows narrower than 128 floats, a forced 6 or 8 rows, K1."""
import collections

import aggregate_ref as ar
import bf16_wide_ref as bw


def test_the_mirror_row_counts_are_the_instantiated_kernels():
    """the mirror's row counts against the kernels in the built library (not against the wording of the sources); that the dispatch
    takes the form exactly where the mirror says is what the counters in tests/test_gpu_bf16_wide_gather.py decide"""
    from test_bf16_wide_resources import _wide_kernels
    assert sorted({r for r, _ in _wide_kernels()}) == list(bw.WIDE_ROWS) and bw.WIDE_MIN_LD == 128


def test_the_sixty_nine_wide_aggregations_by_name():
    ag = bw.wide_aggregations()
    got = collections.defaultdict(dict)
    for case, direction, _, form in ag:
        got[case[0]][direction] = form["R"]
    assert {cid: set(v.values()) for cid, v in got.items()} == {cid: {r} for cid, r in bw.EXPECTED.items()}
    assert all(set(v) == set(ar.DIRECTIONS) for v in got.values())
    assert len(ag) == 69 and len(got) == 23
    rows = collections.Counter(form["R"] for *_, form in ag)
    assert rows == {2: 51, 3: 6, 4: 9, 5: 3}, rows
    assert sum(f["two_launches"] for *_, f in ag) == 18
    assert sum(f["pieces"] for *_, f in ag) == 18
    assert sum(f["max_pieces"] > 200 for *_, f in ag) == 12
    assert sum(f["spp"] > 1 for *_, f in ag) == 6
    assert sum(f["N"] == 8 for *_, f in ag) == 3
    # rows of 128 floats or more only, K1s on bf16 rows only
    assert all(rec["ld"] >= 128 and rec["family"] == "k1s" and rec["bf16"] for _, _, rec, _ in ag)
    # several slabs (F = 602: five, F = 300: three, F = 256: two) and one
    assert {f["slabs"] for *_, f in ag} == {1, 2, 3, 5}
    # a layout made for 16-lane groups (spmm_blk_group = 16) takes the wide form on fewer slabs than its narrow launches
    g16 = [(rec, f) for c, _, rec, f in ag if c[0] == "planted_F300_g16"]
    assert g16 and all(rec["group"] == 16 and rec["slabs"] == 5 and f["slabs"] == 3 for rec, f in g16)


def test_every_instantiated_wide_form_is_reached():
    """(R, loader): the loader wave is walked inside every case (spmm_sweep_loader 1 / 0), so every row count runs both"""
    ag = bw.wide_aggregations()
    reached = set()
    for case, direction, _, _ in ag:
        for loader in (1, 0):
            _, form, why = bw.wide_record(case, direction, {"spmm_sweep_loader": loader})
            assert form, (case[0], direction, why)
            reached.add((form["R"], form["loader"]))
    assert reached == {(r, l) for r in bw.WIDE_ROWS for l in (True, False)}
    # the other schedules of the walk keep the form
    for case, direction, _, base in ag:
        for extra in ({"spmm_blk_force_split": 1}, {"spmm_order": 0}, {"spmm_order": 2}):
            _, form, _ = bw.wide_record(case, direction, extra)
            assert form == base, (case[0], direction, extra)


def test_option_off_and_fp32_rows_run_as_before():
    for case in ar.CASES:
        for direction in ar.DIRECTIONS:
            assert bw.wide_record(case, direction, wide_option=0)[1] is None
            assert bw.wide_record(case, direction, {"gcn_bf16_gather": 0})[1] is None
            rec, form, _ = bw.wide_record(case, direction, {"gcn_bf16_gather": 1})     # forward only
            assert form is None or direction != "bwd"


def test_the_fallbacks_are_reached():
    seen = set()
    for cid, extra, why in bw.FALLBACKS:
        case = bw.case_by_id(cid)
        for direction in ar.DIRECTIONS:
            rec, form, reason = bw.wide_record(case, direction, extra)
            assert form is None, (cid, extra, direction)
            if why == "k1":
                assert rec["family"] == "k1" and reason.startswith("not K1s"), (cid, reason)
            elif why == "ld < 128":
                assert rec["family"] == "k1s" and rec["bf16"] and rec["ld"] < 128 and reason == "ld < 128", (cid, reason)
            else:
                forced = extra["spmm_sweep_rows"]
                assert rec["family"] == "k1s" and rec["bf16"] and rec["ld"] >= 128 and forced in (6, 8), (cid, reason)
                assert reason == f"16-lane row count {forced} not instantiated", (cid, reason)
                assert rec["R"] == forced                     # the narrow launch takes the forced rows on its 32 lanes
                seen.add(forced)
            seen.add(why)
    assert seen == {"k1", "ld < 128", "forced", 6, 8}
    assert {bw.case_by_id(c)[2] for c, _, w_ in bw.FALLBACKS if w_ != "forced"} >= {41, 64}
