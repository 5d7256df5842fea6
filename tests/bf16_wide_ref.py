"""Option gcn_bf16_wide (include/dorylus_hip.h): the Python mirror of the rule by which spmm_k1s (csrc/abi_stages.hip) takes the
wide form of K1s on bf16 rows -- sweep_wide_applies in csrc/spmm.hip -- on top of aggregate_ref.dispatch, and the aggregations of
aggregate_ref.CASES that take it.  tests/test_bf16_wide_reference.py proves what the list reaches where there is no GPU;
tests/test_gpu_bf16_wide_gather.py runs it."""
import aggregate_ref as ar

WIDE_ROWS = (2, 3, 4, 5)                          # the instantiated row counts of spmm_sweep_bf16x8_kernel (loader on and off each)
WIDE_MIN_LD = 128


def wide_form(rec, wide_option=1, cus=ar.CUS_PER_XCD):
    """None where the aggregation of dispatch record `rec` runs as before (with the reason as a second value), else what the wide
    launch looks like: 16-lane groups, R rows per group, slabs of 128 features"""
    if rec["family"] != "k1s":
        return None, "not K1s: " + rec["family"]
    if not rec["bf16"]:
        return None, "fp32 rows"
    if wide_option != 1:
        return None, "option off"
    if rec["ld"] < WIDE_MIN_LD:
        return None, "ld < 128"
    if rec["group"] not in (16, 32):
        return None, "lane group"
    R = ar.sweep_rows_for(rec["layout_R"], 16, min(32, cus), rec["options"]["spmm_sweep_rows"])
    if R not in WIDE_ROWS:
        return None, f"16-lane row count {R} not instantiated"
    RW = ar.SWEEP_NT // 16 * R
    rpx = ar._cdiv(ar._cdiv(rec["npos"], 8), R) * R
    tiles_x = ar._cdiv(rpx, RW)
    return dict(R=R, loader=rec["loader"], slabs=ar._cdiv(rec["ld"] // 8, 16), spp=ar._cdiv(tiles_x, min(32, cus)),
                two_launches=rec["two_launches"], pieces=rec["pieces"], max_pieces=rec["max_pieces"], N=rec["N"]), None


def wide_record(case, direction, extra=None, wide_option=1):
    """(dispatch record, wide form or None, reason) of one aggregation of a case with family k1s asked for and gcn_bf16_gather = 2
    unless `extra` says otherwise"""
    o = {"gcn_bf16_gather": 2}
    o.update(extra or {})
    family = {v: k for k, v in ar.FAMILIES.items()}[o.pop("spmm_variant", 2)]
    rec = ar.case_record(case, family, direction, o)
    form, why = wide_form(rec, wide_option)
    return rec, form, why


def wide_aggregations():
    """[(case, direction, dispatch record, wide form)]: the aggregations of CASES x DIRECTIONS that take the wide form"""
    out = []
    for case in ar.CASES:
        for direction in ar.DIRECTIONS:
            rec, form, _ = wide_record(case, direction)
            if form:
                out.append((case, direction, rec, form))
    return out


# the 69 aggregations (23 cases x 3 directions) the list holds, by name with their 16-lane row count: a change to
# aggregate_ref.CASES cannot silently shrink what the GPU test covers
EXPECTED = {
    "multi_F128_nb8": 2, "multi_F602_nb16": 2, "u1025_F128": 2, "u20k_F128": 2, "u33k_F128": 3, "u120k_F128": 4, "u70001_F128": 5,
    "u70001_F128_r2": 2, "u33k_F256_layout0": 3, "staging_F128": 4, "n8": 4, "powerlaw_F128": 2, "powerlaw_F602": 2,
    "planted_F128": 2, "planted_F300_g16": 2, "hubs_F128": 2, "hubs_F602": 2, "ghosts_small_F128": 2, "ghosts_small_F128_nb2": 2,
    "ghosts_big_F128": 2, "ghosts_big_F602": 2, "ghosts_big_F300_nb24": 2, "ghosts_unread_F128": 2,
}

# aggregations that must NOT take the wide form although gcn_bf16_gather = 2 and gcn_bf16_wide = 1: (case id, options on top of the
# case's -- set before the upload, as the case's own --, why)
FALLBACKS = [
    ("u33k_F64", {}, "ld < 128"), ("u20k_F64", {}, "ld < 128"), ("hubs_F41", {}, "ld < 128"),   # F = 64 and F = 41 on K1s
    ("multi_F41", {}, "k1"),                                                                     # F = 41 on K1
    ("u33k_F128", {"spmm_sweep_rows": 6}, "forced"), ("u33k_F128", {"spmm_sweep_rows": 8}, "forced"),   # no wide <16,6> / <16,8>
    ("u120k_F128", {"spmm_sweep_rows": 6}, "forced"), ("ghosts_big_F602", {"spmm_sweep_rows": 8}, "forced"),
    ("u33k_F128", {"spmm_variant": 0}, "k1"), ("ghosts_big_F602", {"spmm_variant": 0}, "k1"),    # K1 asked for
    ("multi_F602", {}, "k1"),                                                                    # an L2-sized graph without a block count: K1
]


def case_by_id(cid):
    return next(c for c in ar.CASES if c[0] == cid)
