"""dory_set_option / dory_get_option on a context against the table they are driven by (dorylus_amd/host/options.cpp, read through
dory_option_spec): defaults, read-only keys, unknown keys, a round trip of every option, and the refusals that depend on the
context's state -- the uploaded graph (on the smallest one there is: 8 vertices) and the configured model."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DIMS, V = [4, 4, 2], 8


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


@pytest.fixture(scope="module")
def specs(da):
    return da.option_specs()


@pytest.fixture(scope="module")
def fresh(da):
    """a context nobody configured; every test leaves its options as it found them"""
    ctx = da.Context(0)
    yield ctx
    ctx.close()


def _options(da, specs):
    return [s for s in specs if s["kind"] == da._lib.OPTION]


def test_fresh_context_reads_the_table_defaults(da, specs, fresh):
    assert len(_options(da, specs)) == 38
    for s in _options(da, specs):
        assert fresh.get_option(s["name"]) == s["default"], s["name"]


def test_read_only_keys_read_and_refuse_a_set(da, specs, fresh):
    ro = [s["name"] for s in specs if s["kind"] == da._lib.READ_ONLY]
    assert len(ro) == 25
    for name in ro:
        assert isinstance(fresh.get_option(name), int)
        with pytest.raises(da.DoryError, match="unknown option '%s'" % name):
            fresh.set_option(name, 0)
    assert fresh.get_option("spmm_gates_rearm") == 0     # the action reads "is a back-off pending"
    fresh.set_option("spmm_gates_rearm", 1)


def test_unknown_key(da, fresh):
    with pytest.raises(da.DoryError, match="unknown option 'spmm_varient'"):
        fresh.set_option("spmm_varient", 1)
    with pytest.raises(da.DoryError, match="unknown option 'spmm_varient'"):
        fresh.get_option("spmm_varient")
    with pytest.raises(da.DoryError, match="unknown option 'spmm_varient'"):   # the miss did not make it known
        fresh.get_option("spmm_varient")


def test_every_option_round_trips(da, specs, fresh):
    for s in _options(da, specs):
        name = s["name"]
        value = 1 if name == "spmm_sweep_cus" else s["hi"] if s["lo"] <= s["hi"] else s["default"] + 1
        assert value != s["default"]
        fresh.set_option(name, value)
        assert fresh.get_option(name) == value, name
        fresh.set_option(name, s["default"])
        assert fresh.get_option(name) == s["default"], name
    for s in _options(da, specs):                         # ... and no set touched another option
        assert fresh.get_option(s["name"]) == s["default"], s["name"]


def test_refusals_by_model_and_graph(da):
    from helpers import random_graph
    import partition_oracle as po
    src, dst = random_graph(1, V, 16)
    g = po.preprocess(src, dst, np.zeros(V, np.int64), 0, 1)
    with da.Context(0) as ctx:
        # the model: an option of another model that is on refuses the configure; a configured model refuses the option
        ctx.set_option("gatmh_bf16_wide", 1)
        with pytest.raises(da.DoryError, match=r"dory_configure: gatmh_bf16_wide is an option of the multi-head GAT \(set it to 0 first\)"):
            ctx.configure(da.GCN, DIMS, V)
        ctx.set_option("gatmh_bf16_wide", 0)
        ctx.configure(da.GATMH, DIMS, V)
        with pytest.raises(da.DoryError, match="gcn_bf16_gather: GCN contexts only"):
            ctx.set_option("gcn_bf16_gather", 1)
        assert ctx.get_option("gcn_bf16_gather") == 0
        ctx.set_option("gcn_bf16_gather", 0)
        ctx.set_option("gatmh_bf16_wide", 1)
        ctx.set_option("gatmh_bf16_wide", 0)
        # the graph: two options are fixed by the upload, the others are not
        ctx.configure(da.GCN, DIMS, V)
        ctx.set_option("halo_direct_recv", 0)
        ctx.set_option("spmm_sweep_cus", 0)
        ctx.graph_upload(g)
        with pytest.raises(da.DoryError, match=r"halo_direct_recv: set it before the graph is uploaded \(the adjacency's ghost numbering depends on it\)"):
            ctx.set_option("halo_direct_recv", 1)
        with pytest.raises(da.DoryError, match="spmm_sweep_cus: set it before the graph is uploaded$"):
            ctx.set_option("spmm_sweep_cus", 1)
        assert ctx.get_option("halo_direct_recv") == 0 and ctx.get_option("spmm_sweep_cus") == 0
        ctx.set_option("gcn_cache_ah0", 1)
        assert ctx.get_option("gcn_cache_ah0") == 1
