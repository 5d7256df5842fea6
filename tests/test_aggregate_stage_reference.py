"""The float64 reference of the aggregation stage (tests/aggregate_ref.py) against the committed C oracle, the exactness premise
of every case, the mirror's constants against the sources, and the proof that the case list of tests/test_gpu_aggregate_stage.py
reaches every form of K1, K1b and K1s -- what the GPU test relies on, checked where there is no GPU."""
import os
import re

import numpy as np
import pytest

import aggregate_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dorylus_amd", "csrc")
GRAPHS = sorted({c[1] for c in ar.CASES} | {c[1] for c in ar.UNIT_CASES})


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _one(src, pattern):
    m = re.findall(pattern, src)
    assert len(m) == 1, (pattern, m)
    return m[0]


@pytest.mark.parametrize("gname", GRAPHS)
@pytest.mark.parametrize("direction", ["fwd0", "bwd"])
def test_reference_matches_the_c_oracle(gname, direction):
    """aggregate() in float64 against orc.aggregate_gcn (fp32, edge order) on real inputs: every element inside the bound an
    fp32 sum of n + 1 terms has in any order -- which is at once the check that the bound holds for the one fp32
    implementation that runs without a GPU"""
    import orc
    g = ar.graph(gname, "real")
    ptr, idx, val, _ = ar.side(g, direction)
    F = 33 if int(g["localVtxCnt"]) <= 40000 else 9
    x, xg = ar.features(g, direction, F, exact=False)
    got = orc.aggregate_gcn(ptr, idx, val, g["norm"], x, xg)
    ref = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1)
    bound = ar.fp32_sum_bound(ptr, idx, val, g["norm"], x, xg, 1)
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), (gname, direction, float((err / np.maximum(bound, 1e-300)).max()))
    # the bound is not loose by orders of magnitude: a dropped term of typical size would break it
    rows = np.diff(np.asarray(ptr, np.int64)) > 0
    if rows.any():
        typical = np.abs(val).mean() * np.abs(x).mean()
        assert np.median(bound[rows].max(axis=1)) < typical, (gname, direction)


@pytest.mark.parametrize("gname", GRAPHS)
def test_exact_inputs_are_exact(gname):
    """exact_ok for every graph, side, self mode and the widest row count in use; and the reference on exact inputs is made of
    multiples of 1/4 that fp32 holds"""
    g = ar.graph(gname)
    for direction in ("fwd0", "bwd"):
        ptr, idx, val, _ = ar.side(g, direction)
        x, xg = ar.features(g, direction, 8, exact=True)
        for mode in (0, 1, 2):
            ar.exact_ok(ptr, idx, val, g["norm"], x, xg, mode)
        ref = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1)
        assert (ref * 4 == np.rint(ref * 4)).all() and (ref.astype(np.float32).astype(np.float64) == ref).all()
        assert (ar.bf16_round(x) == x).all()
    # CSC and CSR describe the same local-local edges
    N = int(g["localVtxCnt"])
    a = ar._matrix(g["colPtr"], g["rowIdx"], g["cscVal"], N + int(g["srcGhostCnt"]))[:, :N]
    b = ar._matrix(g["rowPtr"], g["colIdx"], g["csrVal"], N + int(g["dstGhostCnt"]))[:, :N]
    assert abs(a - b.T).max() == 0 if a.nnz else b.nnz == 0


def test_exact_ok_refuses_what_is_not_exact():
    g = ar.graph("uniform:1025:12000")
    ptr, idx, val, _ = ar.side(g, "fwd0")
    x, _ = ar.features(g, "fwd0", 4, exact=True)
    with pytest.raises(AssertionError):
        ar.exact_ok(ptr, idx, val * np.float32(3), g["norm"], x, None, 1)
    with pytest.raises(AssertionError):
        ar.exact_ok(ptr, idx, val, g["norm"], x + np.float32(0.5), None, 1)
    with pytest.raises(AssertionError):        # a row whose magnitude leaves the 22 bits
        big = np.zeros(2 ** 19 + 1, np.uint64)
        big[1:] = np.arange(1, 2 ** 19 + 1)
        ar.exact_ok(np.array([0, 2 ** 19], np.uint64), np.zeros(2 ** 19, np.uint32), np.full(2 ** 19, 2, np.float32), np.ones(1, np.float32),
                    np.full((1, 1), 8, np.float32), None, 0)


def test_reference_by_hand():
    ptr, idx, val = np.array([0, 2, 2, 5]), np.array([1, 3, 0, 0, 4]), np.array([0.5, -2, 1, 1, 0.25])
    xl, xg = np.array([[1.0], [2.0], [3.0]]), np.array([[4.0], [8.0]])
    assert ar.aggregate(ptr, idx, val, [2, 2, -1], xl, xg, 1).ravel().tolist() == [2 + 1 - 8, 4, -3 + 1 + 1 + 2]
    assert ar.aggregate(ptr, idx, val, None, xl, xg, 0).ravel().tolist() == [-7, 0, 4]
    assert ar.aggregate(ptr, idx, val, None, xl, xg, 2).ravel().tolist() == [-6, 2, 7]
    assert ar.magnitude(ptr, idx, val, [2, 2, -1], xl, xg, 1).ravel().tolist() == [2 + 1 + 8, 4, 3 + 1 + 1 + 2]
    assert ar.bf16_round(np.float32([1.0, 257.0, 1 + 2 ** -8, 1 + 3 * 2 ** -8])).tolist() == [1.0, 256.0, 1.0, 1 + 2 ** -6]


def test_mirror_constants_match_the_sources():
    """if this fails a kernel was retuned: update the mirror, then look at what the case list still reaches
    (test_case_list_reaches_every_form)"""
    ctx, spmm, blk, core, stages = _src("ctx.hpp"), _src("spmm.hip"), _src("spmm_blocked.hip"), _src("sweep_core.hpp"), _src("abi_stages.hip")
    geo, rows = _src("sweep_geometry.hpp"), _src("../host/sweep_geometry.cpp")
    m = re.search(r"constexpr uint32_t LONG_ROW_CLAMP = (\d+), LONG_ROW_CHUNK = (\d+);", ctx)
    assert (int(m[1]), int(m[2])) == (ar.LONG_ROW_CLAMP, ar.LONG_ROW_CHUNK)
    m = re.search(r"constexpr uint32_t BLK_SEG_CLAMP = (\d+), BLK_SEG_CHUNK = (\d+);", ctx)
    assert (int(m[1]), int(m[2])) == (ar.BLK_SEG_CLAMP, ar.BLK_SEG_CHUNK)
    assert int(_one(ctx, r"inline uint32_t pad_ld\(uint32_t cols\) \{ return cols <= 1 \? cols : \(cols \+ (\d+)u\) & ~31u; \}")) == 31
    assert int(_one(spmm, r"constexpr uint32_t SWEEP_SPLIT = (\d+);")) == ar.SWEEP_SPLIT
    assert int(_one(spmm, r"split_deg = std::max<uint64_t>\((\d+), \(uint64_t\)SWEEP_SPLIT \* \(nnz / N \+ 1\)\);")) == ar.SWEEP_SPLIT_MIN
    assert int(_one(core, r"constexpr int SWEEP_C = (\d+);")) == ar.SWEEP_C
    assert int(_one(geo, r"constexpr int SWEEP_NT = (\d+);")) == ar.SWEEP_NT
    assert "CE = C - 1" in core                      # a pass holds SWEEP_C - 1 entries
    assert int(_one(blk, r"constexpr int BLK_ROWS = (\d+);")) == ar.BLK_ROWS
    # the "tiny" rule of both layouts, the block-count and offset-table limits
    assert len(re.findall(r"\(uint64_t\)NG \* group \* 16u <= \(\(uint64_t\)(\d+) << 20\)", stages)) == 2
    assert {int(x) << 20 for x in re.findall(r"\(uint64_t\)NG \* group \* 16u <= \(\(uint64_t\)(\d+) << 20\)", stages)} == {ar.TINY_BYTES}
    assert int(_one(stages, r"if \(tiny \|\| nb > (\d+) \|\|")) == ar.BLOCKED_MAX_NB
    assert int(_one(stages, r"if \(tiny \|\| c->N < 8 \|\| \(want_nb \? want_nb : nb_est\) > (\d+) \|\|")) == ar.SWEEP_MAX_NB
    assert {int(x) << 30 for x in re.findall(r"\* 8ull > \(\(uint64_t\)(\d+) << 30\)", stages)} == {ar.OFFSET_TABLE_BYTES}
    # the window sizes
    m = re.search(r"\(R <= 4 \? (\d+)u : (\d+)u\)\);", stages)
    assert (int(m[1]), int(m[2])) == (ar.SWEEP_WINDOW_KB_FEW_ROWS, ar.SWEEP_WINDOW_KB)
    assert "nb_est = ((uint64_t)NG * group * 16u + window - 1) / window + 1;" in stages
    m = re.search(r"row_bytes >= 512 \? \(uint64_t\)(\d+)u : \(uint64_t\)(\d+)u;", blk)
    assert (int(m[1]), int(m[2])) == (ar.BLOCKED_WINDOW_WIDE, ar.BLOCKED_WINDOW_NARROW)
    assert "if (ld < 128 && group == 32) group = 16;" in stages
    # launch_spmm's chunk table, in order
    table = [(int(a), int(b), int(c)) for a, b, c in re.findall(r"if \(ch <= (\d+)\) return launch_t<(\d+), (\d+)>\(a, s, bf16\);", spmm)]
    last = re.search(r"\n    return launch_t<(\d+), (\d+)>\(a, s, bf16\);", spmm)
    assert table + [(None, int(last[1]), int(last[2]))] == ar.K1_TABLE
    # sweep_pick_r's candidates and rules; the instantiated (GROUP, R)
    assert [int(x) for x in _one(rows, r"for \(int R : \{([\d, ]+)\}\)").split(",")] == ar.PICK_R
    assert "if (fill > best_fill + 0.02) { best_fill = fill; best = R; }" in rows
    assert "if (rows_per_group && group == 16) return std::max<int>(2, (int)rows_per_group / 2);" in rows
    inst = set()
    for g in (32, 16):   # k1s_narrow_form: the row counts each lane-group width is instantiated for
        picked = _one(spmm, r"group == %d\)? (?:return|&&) sweep_pick<([\d, ]+)>\(R, \[&\]\(auto RR\) \{ return f\(std::integral_constant<int, %d>" % (g, g))
        inst |= {(g, int(r)) for r in picked.split(",")}
    assert inst == {(32, 10)} | {(16, 5), (16, 3)} | {(g, r) for g in (16, 32) for r in (8, 6, 4, 2)}
    assert inst == set(ar.K1S_FORMS)
    # the defaults of the options the mirror reads: what the built library's table reports (dory_option_spec)
    from dorylus_amd import _lib as L
    defaults = {s["name"]: s["default"] for s in L.option_specs() if s["kind"] == L.OPTION}
    assert defaults["spmm_sweep_loader_relief"] == ar.LOADER_RELIEF
    for key, v in ar.DEFAULTS.items():
        assert defaults[key] == v, key


def test_mirror_by_hand():
    """values worked out by hand from the sources"""
    assert [ar.sweep_pick_r(n, 32, 32, 0) for n in (1025, 20000, 33000, 120000, 70001)] == [2, 4, 6, 8, 10]
    assert ar.sweep_pick_r(33000, 16, 32, 3) == 3 and ar.sweep_pick_r(33000, 32, 32, 3) == 6 and ar.sweep_pick_r(33000, 16, 32, 10) != 10
    assert [ar.sweep_rows_for(r, 16, 32, 0) for r in (2, 4, 6, 8, 10)] == [2, 2, 3, 4, 5]
    assert ar.sweep_rows_for(8, 32, 32, 3) == 8 and ar.sweep_rows_for(8, 16, 32, 3) == 3
    assert [ar.k1_form(ld, 0) for ld in (32, 64, 128, 256, 320, 512, 608, 1440)] == \
        [(8, 1, 1), (16, 1, 1), (32, 1, 1), (64, 1, 1), (32, 3, 1), (64, 2, 1), (64, 3, 1), (64, 4, 2)]
    assert ar.k1_form(608, 64) == (16, 1, 10)
    assert ar.split_deg(1000, 100) == 64 and ar.split_deg(4000000, 100000) == 82
    # 20 000 rows of 12 edges: no pieces, R = 4; one sweep of 8 x 32 x 32 groups of 4 rows holds 32 768 positions
    assert ar.deal_npos(20000, 4, 32, 0) == 32768 and ar.deal_npos(120000, 8, 32, 0) == 8 * 2 * 1024 * 8
    ptr = np.arange(0, 20001 * 12, 12)
    rec = ar.dispatch(20000, 0, 128, ptr, np.zeros(240000, np.int64))
    assert (rec["family"], rec["group"], rec["R"], rec["nb"], rec["spp"], rec["pair"]) == ("k1s", 32, 4, 3 + 0, 1, False)
    rec = ar.dispatch(20000, 0, 128, ptr, np.zeros(240000, np.int64), {"spmm_variant": 1})
    assert (rec["family"], rec["nb"], rec["rounds"], rec["long_segments"]) == ("k1b", 8, 1, False)
    rec = ar.dispatch(5000, 0, 128, np.arange(0, 5001 * 12, 12), np.zeros(60000, np.int64))
    assert rec["family"] == "k1"                  # 5 000 x 512 bytes: the slab fits one L2
    rec = ar.dispatch(20000, 0, 128, ptr, np.zeros(240000, np.int64), {"gcn_bf16_gather": 1, "spmm_variant": 1})
    assert rec["family"] == "k1" and rec["bf16"]


def test_planted_rows_sit_on_the_boundaries():
    """every boundary the kernels have is the exact degree of a row, on both sides"""
    want_short = [0, 1, 3, 4, 5] + [g + k for g in (8, 16, 32, 64) for k in (-1, 0, 1)] + [ar.SWEEP_C + k for k in (-2, -1, 0, 1)]
    g = ar.graph("planted")
    for sidename, direction in (("in", "fwd0"), ("out", "bwd")):
        ptr, idx, _, _ = ar.side(g, direction)
        deg = np.diff(ptr.astype(np.int64))
        for v, d in g["planted"][sidename].items():
            assert deg[v] == d, (sidename, v, d)
        have = set(g["planted"][sidename].values())
        sd = ar.split_deg(int(ptr[-1]), int(g["localVtxCnt"]))
        assert sd > 64                              # (not the same row as GROUP = 64)
        assert set(want_short) | {sd, sd + 1} <= have
        assert {ar.BLK_SEG_CLAMP, ar.BLK_SEG_CLAMP + 1, ar.BLK_SEG_CLAMP + ar.BLK_SEG_CHUNK, ar.BLK_SEG_CLAMP + ar.BLK_SEG_CHUNK + 1} <= have
        assert deg.max() <= ar.LONG_ROW_CLAMP       # this graph keeps the edge split and the row split of K1
        # the segment rows' edges lie in one source block of K1b's layout (whatever the block count in use)
        for nb in (8, 16, 24):
            SB = -(-int(g["localVtxCnt"]) // nb)
            for v, d in g["planted"][sidename].items():
                if d >= ar.BLK_SEG_CLAMP:
                    assert np.unique(idx[ptr[v]:ptr[v + 1]] // SB).size == 1
    g = ar.graph("hubs")
    C, K = ar.LONG_ROW_CLAMP, ar.LONG_ROW_CHUNK
    for sidename, direction in (("in", "fwd0"), ("out", "bwd")):
        ptr, _, _, _ = ar.side(g, direction)
        deg = np.diff(ptr.astype(np.int64))
        for v, d in g["planted"][sidename].items():
            assert deg[v] == d
        have = set(g["planted"][sidename].values())
        assert {C, C + 1, C + 2, C + 3, C + K, C + K + 1, C + K + 2, C + K + 3} <= have       # chunks of 1, 2 and 3 edges: waves with nothing
        assert any(d > C + K and (d - C) % K % 4 for d in have)
        sd = ar.split_deg(int(ptr[-1]), int(g["localVtxCnt"]))
        assert sd == ar.SWEEP_SPLIT_MIN and ar.HUNDREDS_OF_PIECES * sd in have
        assert (deg == 0).mean() > 0.6              # many empty rows
    # one lane group's entries of one step around a staging pass of SWEEP_C - 1 entries (SWEEP_C / 2 - 1 on 16 lanes with the
    # loader): graph "staging" in row order over one source block, four rows per group, no pieces
    g = ar.graph("staging")
    for sidename, direction in (("in", "fwd0"), ("out", "bwd")):
        ptr, idx, _, _ = ar.side(g, direction)
        deg = np.diff(ptr.astype(np.int64))
        for v, d in g["planted"][sidename].items():
            assert deg[v] == d
        assert deg.max() <= ar.split_deg(int(ptr[-1]), 4096) == 64
        for F in (128, 64):
            case = ar.CASES[ar.CASE_IDS.index(f"staging_F{F}")]
            rec = ar.case_record(case, "k1s", direction)
            assert (rec["family"], rec["R"], rec["nb"], rec["pieces"], rec["npos"]) == ("k1s", 4, 1, False, 4096)
        sums = set(ar.group_step_entries(deg, 4).tolist())
        assert {ar.SWEEP_C + k for k in (-2, -1, 0, 1)} | {ar.SWEEP_C // 2 + k for k in (-2, -1, 0, 1)} <= sums


def test_case_list_reaches_every_form():
    """the counterpart of test_case_list_covers_the_plan: over the GPU case list (cases x families x directions x the walked
    schedules, and the unit-weight cases) the mirror reports every form of K1, K1b and K1s; what the dispatch cannot reach is
    named with its reason"""
    got = ar.covered_forms()
    missing = [f for f in ar.REQUIRED_FORMS if f not in got]
    assert not missing, missing
    for f in ar.UNREACHABLE_FORMS:
        assert f not in got and f.split("+")[0].split("*")[0] != "", f
    # nothing the mirror can report is left out of both lists, apart from forced forms that are also reached by the pick
    extra = {f for f in got if f not in ar.REQUIRED_FORMS}
    assert all(":forced" in f for f in extra), sorted(extra)
    # every family asked for runs somewhere, and the fall-through (a family asked for, the next one taken) occurs too
    ran = {(fam, ar.case_record(c, fam, "fwd0")["family"]) for c in ar.CASES for fam in ar.FAMILIES}
    assert {("k1", "k1"), ("k1b", "k1b"), ("k1s", "k1s"), ("k1s", "k1"), ("k1b", "k1"), ("k1s", "k1b")} <= ran, ran


def test_case_sizes():
    """graphs of at most 2.5 M edges; wide rows only on graphs of a few tens of thousands of rows"""
    for _, gname, F, _ in ar.CASES + ar.UNIT_CASES:
        g = ar.graph(gname)
        assert max(len(g["rowIdx"]), len(g["colIdx"])) <= 2_500_000
        assert F <= 300 or int(g["localVtxCnt"]) <= 30000, (gname, F)
    assert len(set(ar.CASE_IDS)) == len(ar.CASE_IDS)
