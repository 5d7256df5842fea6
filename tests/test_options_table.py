"""The table of the context's options and read-only keys (dorylus_amd/host/options.cpp) through dory_option_spec and
dory_option_check: names, defaults, ranges, model and graph refusals with their texts.  No GPU.  The expected values are
literals: the table must reproduce what dory_create and dory_set_option did before the options had one owner."""
import pytest

from dorylus_amd import _lib as L

DEFAULTS = {
    "spmm_variant": 2, "spmm_sweep_flags": 0, "spmm_sweep_rows": 0, "spmm_sweep_pair": -1, "spmm_sweep_loader": 1,
    "spmm_sweep_loader_relief": 3, "spmm_sweep_reserve_cus": 4, "spmm_sweep_layout": 3, "spmm_sweep_window_kb": 0,
    "spmm_xcd_assume_mismatch": 0, "spmm_slab": 0, "spmm_order": 1, "spmm_blk_group": 32, "spmm_blk_force_split": 0,
    "halo_overlap": 1, "gat_lazy_edge_tensors": 1, "gat_reuse_nsum": 1, "spmm_edge_split": 1, "spmm_sweep_cus": 0,
    "local_timeout_ms": 30000, "adjacency_values_asymmetric": 0, "gatmh_bwd_phase": 0, "gatmh_blocked": 1,
    "gatmh_el_on_the_fly": 1, "gatmh_sweep": 1, "gatmh_src_window_kb": 0, "gatmh_sweep_rows": 0, "gatmh_fused_stats": 1,
    "gcn_cache_ah0": 0, "gcn_bf16_gather": 0, "gcn_bf16_wide": 0, "gatmh_bf16_gather": 0, "gatmh_bf16_wide": 0,
    "halo_exact_rows": 0, "halo_direct_recv": 0, "gcn_transform_first": 0, "epoch_graph": 0, "spmm_blk_nb": 0,
}
READ_ONLY = [
    "gcn_cache_ah0_skips", "gcn_bf16_gathers_k1s", "gcn_bf16_gathers_k1s_wide", "gcn_bf16_gathers_k1",
    "spmm_launches_k1s", "spmm_launches_k1b", "spmm_launches_k1",
    "gatmh_bf16_gathers_fwd", "gatmh_bf16_gathers_src", "gatmh_bf16_gathers_fwd_wide", "gatmh_bf16_gathers_src_wide",
    "halo_rows_packed", "halo_floats_packed", "halo_exact_packs", "halo_direct_recvs", "halo_staged_recvs", "halo_recv_buf_bytes",
    "epoch_graph_recorded",
    "spmm_xcd_mapping_ok", "spmm_xcd_count", "spmm_xcd_policy", "spmm_xcd_gated_us", "spmm_xcd_ungated_us",
    "spmm_gate_timeouts", "spmm_ungated_launches",
]
ACTIONS = ["spmm_gates_rearm"]
# (lo, hi, refusal) of every ranged option: the texts of dory_set_option
RANGES = {
    "gcn_bf16_gather": (0, 2, "gcn_bf16_gather: 0 (off), 1 (forward) or 2 (forward and backward)"),
    "gcn_bf16_wide": (0, 1, "gcn_bf16_wide: 0 (off) or 1 (16-byte gathers of bf16 rows in K1s)"),
    "gatmh_bf16_gather": (0, 2, "gatmh_bf16_gather: 0 (off), 1 (forward) or 2 (forward and the backward's source side)"),
    "gatmh_bf16_wide": (0, 1, "gatmh_bf16_wide: 0 (off) or 1 (16-byte gathers of bf16 rows in the multi-head GAT's sweeps)"),
    "halo_exact_rows": (0, 1, "halo_exact_rows: 0 (padded rows travel) or 1 (rows of exactly cols floats)"),
    "halo_direct_recv": (0, 1, "halo_direct_recv: 0 (receive buffer and unpack) or 1 (halo rows land in the ghost tensors, stored in wire order)"),
}
MODEL = {
    "gcn_bf16_gather": (L.GCN, "gcn_bf16_gather: GCN contexts only"),
    "gcn_bf16_wide": (L.GCN, "gcn_bf16_wide: GCN contexts only"),
    "gatmh_bf16_gather": (L.GATMH, "gatmh_bf16_gather: multi-head GAT contexts (DORY_GATMH) only"),
    "gatmh_bf16_wide": (L.GATMH, "gatmh_bf16_wide: multi-head GAT contexts (DORY_GATMH) only"),
}
FIXED = {
    "spmm_sweep_cus": "spmm_sweep_cus: set it before the graph is uploaded",
    "halo_direct_recv": "halo_direct_recv: set it before the graph is uploaded (the adjacency's ghost numbering depends on it)",
}
OK, ERR_ARG = 0, -1
INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def specs(lib):
    return L.option_specs(lib)


def test_options_and_defaults(specs):
    opts = [s for s in specs if s["kind"] == L.OPTION]
    assert len(DEFAULTS) == 38
    assert [(s["name"], s["default"]) for s in opts] == list(DEFAULTS.items())
    assert specs[:len(opts)] == opts                       # options first: their index is their id


def test_keys_that_are_not_options(specs):
    assert len(READ_ONLY) == 25
    assert [s["name"] for s in specs if s["kind"] == L.READ_ONLY] == READ_ONLY
    assert [s["name"] for s in specs if s["kind"] == L.ACTION] == ACTIONS
    assert len(specs) == 38 + 25 + 1
    assert {s["kind"] for s in specs} == {L.OPTION, L.READ_ONLY, L.ACTION}


def test_no_name_twice(specs):
    names = [s["name"] for s in specs]
    assert len(set(names)) == len(names)


def test_only_options_can_be_set(lib):
    for name in READ_ONLY + ACTIONS + ["no_such_option", ""]:
        assert L.option_check(name, 0, lib=lib) == (ERR_ARG, "unknown option '%s'" % name), name
    assert lib.dory_option_check(None, 0, L.GCN, 0, 0, None, 0) == ERR_ARG
    assert lib.dory_option_spec(len(DEFAULTS) + len(READ_ONLY) + 1, *[None] * 8) == ERR_ARG


def test_ranges(lib, specs):
    ranged = {s["name"]: (s["lo"], s["hi"]) for s in specs if s["kind"] == L.OPTION and s["lo"] <= s["hi"]}
    assert ranged == {k: v[:2] for k, v in RANGES.items()}
    for name, (lo, hi, text) in RANGES.items():
        # (an unconfigured context without a graph: nothing but the range can refuse)
        assert L.option_check(name, lo - 1, lib=lib) == (ERR_ARG, text), name
        assert L.option_check(name, lo, lib=lib) == (OK, ""), name
        assert L.option_check(name, hi, lib=lib) == (OK, ""), name
        assert L.option_check(name, hi + 1, lib=lib) == (ERR_ARG, text), name


def test_unranged_options_take_any_value(lib):
    for name in DEFAULTS:
        if name in RANGES:
            continue
        for v in (INT64_MIN, INT64_MAX):
            for gnn in (L.GCN, L.GAT, L.GATMH):
                assert L.option_check(name, v, gnn, True, False, lib=lib) == (OK, ""), (name, v)


def test_model_refusals(lib, specs):
    assert {s["name"]: s["gnn"] for s in specs if s["gnn"] != -1} == {k: v[0] for k, v in MODEL.items()}
    for name, (model, text) in MODEL.items():
        for configured in (False, True):
            for gnn in (L.GCN, L.GAT, L.GATMH):
                refused = configured and gnn != model
                assert L.option_check(name, 1, gnn, configured, lib=lib) == ((ERR_ARG, text) if refused else (OK, "")), (name, configured, gnn)
                assert L.option_check(name, 0, gnn, configured, lib=lib) == (OK, ""), (name, configured, gnn)   # off is always legal
                # the range comes first
                assert L.option_check(name, 3, gnn, configured, lib=lib) == (ERR_ARG, RANGES[name][2])


def test_fixed_by_the_graph(lib, specs):
    assert {s["name"] for s in specs if s["fixed_by_graph"]} == set(FIXED)
    for name, text in FIXED.items():
        for configured in (False, True):
            assert L.option_check(name, 1, L.GCN, configured, False, lib=lib) == (OK, "")
            assert L.option_check(name, 1, L.GCN, configured, True, lib=lib) == (ERR_ARG, text)
            assert L.option_check(name, 0, L.GCN, configured, True, lib=lib) == (ERR_ARG, text)   # whatever the value
    assert L.option_check("halo_direct_recv", 2, L.GCN, True, True, lib=lib) == (ERR_ARG, RANGES["halo_direct_recv"][2])   # range first
    for name in set(DEFAULTS) - set(FIXED):
        assert L.option_check(name, 0, L.GCN, True, True, lib=lib) == (OK, ""), name
