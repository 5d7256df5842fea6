"""ctypes binding of the C-ABI in include/dorylus_hip.h.

There is no CPU fallback: a missing library or a missing gfx950 device raises.
`import torch` (if the caller uses it) must happen before this module loads the
library so that both share one HIP runtime (same SONAME libamdhip64.so.7).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DORY_LIB_PATH") or os.path.join(_HERE, "libdorylus_hip.so")   # DORY_LIB_PATH: A/B runs against another build

# every symbol include/dorylus_hip.h declares (checked by tests/test_abi_symbols.py)
SYMBOLS = [
    "dory_create", "dory_destroy", "dory_last_error", "dory_set_streams", "dory_sync",
    "dory_configure", "dory_graph_upload", "dory_preallocate", "dory_tensor_info",
    "dory_tensor_upload", "dory_tensor_download", "dory_tensor_fill_uniform", "dory_labels_upload",
    "dory_weight_set", "dory_weight_get", "dory_weight_grad_get", "dory_weight_grad_set", "dory_weights_init_xavier",
    "dory_aggregate", "dory_apply_vertex", "dory_apply_edge", "dory_predict_gat", "dory_train_stat", "dory_train_stat_global",
    "dory_halo_plan", "dory_comm_unique_id", "dory_comm_init", "dory_halo_exchange", "dory_halo_pack",
    "dory_halo_unpack", "dory_halo_pack_tensor", "dory_halo_unpack_tensor", "dory_adam_config", "dory_weight_update", "dory_timing_enable",
    "dory_timing_get", "dory_timing_reset", "dory_set_option", "dory_get_option", "dory_ctx_describe",
    "dory_epoch_graph_begin", "dory_epoch_graph_end", "dory_epoch_graph_launch", "dory_epoch_graph_drop",
    "dory_gatmh_heads", "dory_transform_first_active", "dory_transform_first_layer",
    "dory_comm_set_host_transport", "dory_comm_init_local", "dory_debug_occupy_cus",
    "dory_halo_wire_ids", "dory_scatter_msgs_layout", "dory_scatter_msgs_pack", "dory_scatter_msgs_deliver", "dory_scatter_msgs_unpack",
    "dory_scatter_msgs_finish",
    "dory_comm_set_scatter_transport",
    "dory_halo_fused_pack", "dory_halo_fused_pack_stats",
    "dory_gat_bf16_gather", "dory_gat_bf16_gather_stats",
    "dory_halo_bf16_rows", "dory_halo_bf16_rows_stats", "dory_halo_wire_row",
    "dory_halo_bf16_ghosts", "dory_halo_bf16_ghosts_stats", "dory_halo_bf16_ghost_peek",
    "dory_halo_fused_pack_bf16", "dory_halo_fused_pack_bf16_stats",
    "dory_halo_fused_pack_rowwise", "dory_halo_fused_pack_rowwise_stats",
    "dory_gatmh_bwd_merged_exchange", "dory_gatmh_bwd_merged_exchange_stats", "dory_gatmh_bwd_wire_row", "dory_gatmh_bwd_pack",
    "dory_gatmh_bwd_unpack", "dory_gatmh_halo_bf16", "dory_gatmh_halo_bf16_stats", "dory_gatmh_bwd_wire_do",
    "dory_gatmh_row_gather", "dory_gatmh_row_gather_stats",
    "dory_gatmh_row_gather_bf16", "dory_gatmh_row_gather_bf16_stats",
    "dory_gatmh_bf16_ghosts", "dory_gatmh_bf16_ghosts_stats",
    "dory_gatmh_row_gather_hub_split", "dory_gatmh_row_gather_hub_split_stats",
    "dory_gatmh_row_gather_overlap", "dory_gatmh_row_gather_overlap_stats",
    "dory_gatmh_row_gather_edge_split", "dory_gatmh_row_gather_edge_split_stats",
    "dory_gatmh_row_gather_bf16_wide", "dory_gatmh_row_gather_bf16_wide_stats",
    "dory_k1_bf16_wide", "dory_k1_bf16_wide_stats", "dory_k1_bf16_wide_form",
]

# host transport callbacks (include/dorylus_hip.h)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                           C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_uint64)



class ScatterMsg(C.Structure):
    """struct dory_scatter_msg: one message of an exchange inside one buffer"""
    _fields_ = [("peer", C.c_uint32), ("first_row", C.c_uint32), ("rows", C.c_uint32), ("offset", C.c_uint64), ("bytes", C.c_uint64)]


# scatter transport callback (include/dorylus_hip.h)
SCATTER_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ScatterMsg), C.c_uint32)

FORWARD, BACKWARD = 0, 1
GCN, GAT, GATMH = 0, 1, 2


class DoryError(RuntimeError):
    pass


def load():
    if not os.path.exists(LIB_PATH):
        raise DoryError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, u32, u64, i32, f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float
    cp = C.c_char_p
    sig = {
        "dory_create": [i32, C.POINTER(vp)],
        "dory_destroy": [vp],
        "dory_set_streams": [vp, vp, vp],
        "dory_debug_occupy_cus": [vp, u32, u64],
        "dory_sync": [vp],
        "dory_configure": [vp, i32, u32, vp, u32, u32, u32],
        "dory_graph_upload": [vp, u32, u32, u32, u64, vp, vp, vp, u64, vp, vp, vp, vp],
        "dory_preallocate": [vp],
        "dory_tensor_info": [vp, u32, cp, C.POINTER(u64), C.POINTER(u32), C.POINTER(u32), C.POINTER(vp)],
        "dory_tensor_upload": [vp, u32, cp, vp],
        "dory_tensor_download": [vp, u32, cp, vp],
        "dory_tensor_fill_uniform": [vp, u32, cp, u64, f32, f32, vp],
        "dory_labels_upload": [vp, vp],
        "dory_weight_set": [vp, u32, cp, vp],
        "dory_weight_get": [vp, u32, cp, vp],
        "dory_weight_grad_get": [vp, u32, cp, vp],
        "dory_weight_grad_set": [vp, u32, cp, vp],
        "dory_weights_init_xavier": [vp],
        "dory_aggregate": [vp, u32, i32],
        "dory_apply_vertex": [vp, u32, i32],
        "dory_apply_edge": [vp, u32, i32],
        "dory_predict_gat": [vp, u32],
        "dory_train_stat": [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(u32)],
        "dory_train_stat_global": [vp, C.POINTER(f32), C.POINTER(f32), C.POINTER(u32)],
        "dory_halo_plan": [vp, i32, vp, vp, vp, vp],
        "dory_comm_unique_id": [vp],
        "dory_comm_init": [vp, vp, i32, i32],
        "dory_halo_exchange": [vp, u32, i32],
        "dory_halo_pack": [vp, u32, i32, vp],
        "dory_halo_unpack": [vp, u32, i32, vp],
        "dory_halo_pack_tensor": [vp, u32, cp, i32, vp],
        "dory_halo_unpack_tensor": [vp, u32, cp, i32, vp],
        "dory_adam_config": [vp, f32],
        "dory_weight_update": [vp, u32],
        "dory_timing_enable": [vp, i32],
        "dory_timing_get": [vp, cp, C.POINTER(C.c_double), C.POINTER(u64)],
        "dory_timing_reset": [vp],
        "dory_set_option": [vp, cp, C.c_int64],
        "dory_get_option": [vp, cp, C.POINTER(C.c_int64)],
        "dory_transform_first_active": [vp],
        "dory_transform_first_layer": [vp, u32],
        "dory_epoch_graph_begin": [vp], "dory_epoch_graph_end": [vp], "dory_epoch_graph_launch": [vp, u32],
        "dory_epoch_graph_drop": [vp],
        "dory_ctx_describe": [vp, C.POINTER(i32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)],
        "dory_gatmh_heads": [vp, vp],
        "dory_comm_set_host_transport": [vp, ALLTOALLV_FN, ALLREDUCE_FN, vp],
        "dory_comm_init_local": [vp, C.c_uint32],
        # include/dorylus_host.h
        "dory_partition_build": [vp, vp, u64, vp, u32, u32, u32, i32, C.POINTER(vp)],
        "dory_partition_build_from_files": [cp, u32, u32, i32, C.POINTER(vp)],
        "dory_partition_load": [cp, C.POINTER(vp)],
        "dory_partition_save": [vp, cp],
        "dory_partition_free": [vp],
        "dory_partition_get": [vp, vp],
        "dory_partition_upload": [vp, vp, vp],
        "dory_partition_recv_plan": [vp, vp, i32, vp, vp],
        "dory_read_layer_config": [cp, vp, u32, C.POINTER(u32)],
        "dory_read_features": [cp, vp, u32, u32, cp, vp, vp],
        "dory_read_labels": [cp, vp, u32, vp],
        "dory_engine_create": [vp, C.POINTER(vp)],
        "dory_engine_destroy": [vp],
        "dory_engine_run": [vp, u32, vp],
        "dory_engine_nn_compute": [vp, vp],
        "dory_engine_inc_layer": [vp, vp, vp],
        "dory_chunk_inc_layer": [i32, u32, vp, vp],
        "dory_engine_trace_epoch": [i32, u32, C.c_char_p, C.c_size_t],
        "dory_engine_is_last_layer": [vp, vp],
        "dory_engine_report": [vp, cp, C.c_size_t],
        "dory_sweep_deal": [u32, u32, u32, vp, vp, vp],
        "dory_sweep_deal_weighted": [u32, vp, u32, u32, u32, vp, vp, vp],
    }
    # bound only if present: DORY_LIB_PATH may name an older build (an A/B run) from before these entry points
    optional = {
        "dory_halo_wire_ids": [vp, vp, vp, vp],
        "dory_scatter_msgs_layout": [vp, u32, i32, cp, u64, C.POINTER(ScatterMsg), u32, C.POINTER(u32), C.POINTER(u64)],
        "dory_scatter_msgs_pack": [vp, u32, i32, cp, u64, vp],
        "dory_scatter_msgs_deliver": [vp, cp, C.POINTER(vp), C.POINTER(u64), u32],
        "dory_scatter_msgs_unpack": [vp, u32, i32, cp, vp, u32],
        "dory_scatter_msgs_finish": [vp, u32, i32, cp, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)],
        "dory_comm_set_scatter_transport": [vp, SCATTER_EXCHANGE_FN, ALLREDUCE_FN, vp, u64],
        "dory_halo_fused_pack": [vp, i32],
        "dory_halo_fused_pack_stats": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)],
        "dory_gat_bf16_gather": [vp, i32, i32],
        "dory_gat_bf16_gather_stats": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)],
        "dory_halo_bf16_rows": [vp, i32],
        "dory_halo_bf16_rows_stats": [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)],
        "dory_halo_wire_row": [vp, u32, i32, C.POINTER(u32), C.POINTER(u32)],
        "dory_halo_bf16_ghosts": [vp, i32],
        "dory_halo_bf16_ghosts_stats": [vp] + [C.POINTER(u64)] * 5,
        "dory_halo_bf16_ghost_peek": [vp, u32, cp, C.POINTER(vp), C.POINTER(i32)],
        "dory_halo_fused_pack_bf16": [vp, i32],
        "dory_halo_fused_pack_bf16_stats": [vp, C.POINTER(u64), C.POINTER(u64)],
        "dory_halo_fused_pack_rowwise": [vp, i32],
        "dory_halo_fused_pack_rowwise_stats": [vp, C.POINTER(u64), C.POINTER(u64)],
        "dory_gatmh_bwd_merged_exchange": [vp, i32],
        "dory_gatmh_bwd_merged_exchange_stats": [vp] + [C.POINTER(u64)] * 4,
        "dory_gatmh_bwd_wire_row": [vp, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)],
        "dory_gatmh_bwd_pack": [vp, u32, vp],
        "dory_gatmh_bwd_unpack": [vp, u32, vp],
        "dory_gatmh_halo_bf16": [vp, i32],
        "dory_gatmh_halo_bf16_stats": [vp] + [C.POINTER(u64)] * 4,
        "dory_gatmh_bwd_wire_do": [vp, u32, C.POINTER(u32), C.POINTER(u32)],
        "dory_gatmh_row_gather": [vp, i32],
        "dory_gatmh_row_gather_stats": [vp] + [C.POINTER(u64)] * 4,
        "dory_gatmh_row_gather_bf16": [vp, i32],
        "dory_gatmh_row_gather_bf16_stats": [vp] + [C.POINTER(u64)] * 3,
        "dory_gatmh_bf16_ghosts": [vp, i32],
        "dory_gatmh_bf16_ghosts_stats": [vp] + [C.POINTER(u64)] * 7,
        "dory_gatmh_row_gather_hub_split": [vp, u32],
        "dory_gatmh_row_gather_hub_split_stats": [vp] + [C.POINTER(u64)] * 7,
        "dory_gatmh_row_gather_overlap": [vp, i32],
        "dory_gatmh_row_gather_overlap_stats": [vp] + [C.POINTER(u64)] * 7,
        "dory_gatmh_row_gather_edge_split": [vp, i32],
        "dory_gatmh_row_gather_edge_split_stats": [vp] + [C.POINTER(u64)] * 8,
        "dory_gatmh_row_gather_bf16_wide": [vp, i32],
        "dory_gatmh_row_gather_bf16_wide_stats": [vp] + [C.POINTER(u64)] * 4,
        "dory_k1_bf16_wide": [vp, i32],
        "dory_k1_bf16_wide_stats": [vp] + [C.POINTER(u64)] * 2,
        "dory_k1_bf16_wide_form": [u32, u32, C.POINTER(u32), C.POINTER(u32)],
        # include/dorylus_host.h
        "dory_halo_send_map": [u32, u32, vp, vp, vp, vp],
        "dory_row_chunk_plan": [vp, u32, u32, C.POINTER(u32), C.POINTER(u32), vp, vp, vp, vp, vp],
        "dory_row_interior_plan": [vp, vp, u32, C.POINTER(u32), C.POINTER(u32), vp, vp],
        "dory_row_edge_split_plan": [vp, vp, u32, u32, vp, vp],
        "dory_gatmh_row_gather_bf16_wide_form": [u32, u32, u32, C.POINTER(u32), C.POINTER(u32), C.POINTER(i32)],
        "dory_partition_wire_order": [vp, vp, i32, vp, vp],
        "dory_sweep_geometry": [u32, u32, i32, i32, i32, u32, u32, u32, i32, vp],
        "dory_option_spec": [u32, C.POINTER(cp)] + [C.POINTER(t) for t in (i32, C.c_int64, C.c_int64, C.c_int64, i32, i32, i32)],
        "dory_option_check": [cp, C.c_int64, i32, i32, i32, cp, C.c_size_t],
        "dory_switch_spec": [u32, C.POINTER(cp)] + [C.POINTER(i32)] * 6,
        "dory_switch_check": [cp, i32, i32, i32, i32, i32, i32, cp, C.c_size_t],
    }
    for name, args in list(sig.items()) + [(n, a) for n, a in optional.items() if hasattr(lib, n)]:
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = i32
    lib.dory_last_error.argtypes = [vp]
    lib.dory_last_error.restype = cp
    lib.dory_host_last_error.argtypes = []
    lib.dory_host_last_error.restype = cp
    lib.dory_formats_last_error.argtypes = []
    lib.dory_formats_last_error.restype = cp
    return lib


OPTION, READ_ONLY, ACTION = 0, 1, 2     # option_specs()[i]["kind"]


def option_specs(lib=None):
    """The table of the keys of set_option / get_option (dory_option_spec; no context, no GPU): one dict per key with name, kind,
    default, lo, hi (lo > hi: any value), gnn (-1: any model), fixed_by_graph and read (when the library reads it)."""
    lib = lib or load()
    specs = []
    while True:
        name = C.c_char_p()
        kind, gnn, fixed, read = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        default, lo, hi = C.c_int64(), C.c_int64(), C.c_int64()
        if lib.dory_option_spec(len(specs), C.byref(name), C.byref(kind), C.byref(default), C.byref(lo), C.byref(hi), C.byref(gnn),
                                C.byref(fixed), C.byref(read)) != 0:
            return specs
        specs.append({"name": name.value.decode(), "kind": kind.value, "default": default.value, "lo": lo.value, "hi": hi.value,
                      "gnn": gnn.value, "fixed_by_graph": bool(fixed.value), "read": read.value})


def option_check(name, value, gnn=GCN, configured=False, has_graph=False, lib=None):
    """What set_option(name, value) answers on a context of that state (dory_option_check): (return code, refusal text)."""
    lib = lib or load()
    msg = C.create_string_buffer(512)
    rc = lib.dory_option_check(name.encode(), int(value), int(gnn), int(configured), int(has_graph), msg, len(msg))
    return rc, msg.value.decode()


def switch_specs(lib=None):
    """The table of the feature switches Context.<name>(value) (dory_switch_spec; no context, no GPU): one dict per switch with name,
    hi (values 0..hi), refusals (how many its setter has), waits_halo, drops_stamp, parent (index or -1) and counters (of <name>_stats)."""
    lib, specs, name, v = lib or load(), [], C.c_char_p(), [C.c_int() for _ in range(6)]
    while lib.dory_switch_spec(len(specs), C.byref(name), *[C.byref(x) for x in v]) == 0:
        specs.append(dict(zip(("hi", "refusals", "waits_halo", "drops_stamp", "parent", "counters"), (x.value for x in v)), name=name.value.decode()))
    return specs


def switch_check(name, value, gnn=GCN, configured=False, prealloc=False, recording=False, parent_on=False, lib=None):
    """What Context.<name>(value) answers on a context of that state (dory_switch_check): (return code, refusal text)."""
    lib = lib or load()
    msg = C.create_string_buffer(512)
    rc = lib.dory_switch_check(name.encode(), int(value), int(gnn), int(configured), int(prealloc), int(recording), int(parent_on), msg, len(msg))
    return rc, msg.value.decode()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def halo_send_map(local_vtx_cnt, send_lists, lib=None):
    """(row_ptr[N + 1], row_slots[sum of the list lengths]): the send lists of a halo plan (one list of local row ids per peer, as
    Context.halo_plan takes them) turned round -- the slots row r has in the packed send buffer are
    row_slots[row_ptr[r]:row_ptr[r + 1]], ascending (dory_halo_send_map; no context, no GPU)."""
    lib = lib or load()
    sc = np.array([len(x) for x in send_lists], np.uint32)
    sl = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32) for x in send_lists] + [np.zeros(0, np.uint32)]), np.uint32)
    row_ptr, row_slots = np.zeros(int(local_vtx_cnt) + 1, np.uint32), np.zeros(max(sl.size, 1), np.uint32)
    rc = lib.dory_halo_send_map(int(local_vtx_cnt), len(send_lists), _ptr(sc), _ptr(sl), _ptr(row_ptr), _ptr(row_slots))
    if rc != 0:
        raise DoryError(f"dory_halo_send_map failed ({rc}): {lib.dory_host_last_error().decode()}")
    return row_ptr, row_slots[:sl.size]


def row_chunk_plan(ptr, chunk_entries, lib=None):
    """The chunk plan of an adjacency's hub rows (dory_row_chunk_plan; no context, no GPU): ptr = the rows + 1 offsets of a CSR / CSC;
    rows with more than chunk_entries entries are cut into consecutive chunks of chunk_entries entries, the last one shorter.
    Returns (hub_rows, row_first_chunk[len(hub_rows) + 1], chunk_row, chunk_e0, chunk_e1)."""
    lib = lib or load()
    ptr = np.ascontiguousarray(ptr, np.uint64)
    nr, nc = C.c_uint32(), C.c_uint32()
    rc = lib.dory_row_chunk_plan(_ptr(ptr), ptr.size - 1, int(chunk_entries), C.byref(nr), C.byref(nc), None, None, None, None, None)
    if rc != 0:
        raise DoryError(f"dory_row_chunk_plan failed ({rc})")
    rows, first = np.zeros(nr.value, np.uint32), np.zeros(nr.value + 1, np.uint32)
    crow, e0, e1 = np.zeros(nc.value, np.uint32), np.zeros(nc.value, np.uint64), np.zeros(nc.value, np.uint64)
    rc = lib.dory_row_chunk_plan(_ptr(ptr), ptr.size - 1, int(chunk_entries), None, None, _ptr(rows), _ptr(first), _ptr(crow), _ptr(e0), _ptr(e1))
    if rc != 0:
        raise DoryError(f"dory_row_chunk_plan failed ({rc})")
    return rows, first, crow, e0, e1


def row_interior_plan(ptr, idx, N, lib=None):
    """(interior, boundary): the rows of a partition's adjacency (ptr[N + 1], idx; an id >= N names a ghost row) whose entries are all
    local -- a row without entries is one -- and the rows with at least one ghost entry, both ascending (dory_row_interior_plan; no
    context, no GPU).  The plan Context.gatmh_row_gather_overlap builds per adjacency."""
    lib = lib or load()
    ptr, idx = np.ascontiguousarray(ptr, np.uint64), np.ascontiguousarray(idx, np.uint32)
    if ptr.size != int(N) + 1:
        raise DoryError(f"row_interior_plan: ptr has {ptr.size} entries for {N} rows")
    ni, nb = C.c_uint32(), C.c_uint32()
    rc = lib.dory_row_interior_plan(_ptr(ptr), _ptr(idx), int(N), C.byref(ni), C.byref(nb), None, None)
    if rc != 0:
        raise DoryError(f"dory_row_interior_plan failed ({rc})")
    interior, boundary = np.zeros(ni.value, np.uint32), np.zeros(nb.value, np.uint32)
    rc = lib.dory_row_interior_plan(_ptr(ptr), _ptr(idx), int(N), None, None, _ptr(interior), _ptr(boundary))
    if rc != 0:
        raise DoryError(f"dory_row_interior_plan failed ({rc})")
    return interior, boundary


def row_edge_split_plan(ptr, idx, N, lib=None):
    """(idx_local_first, mid): the entries of every row of an adjacency (ptr[rows + 1], idx; an id >= N names a ghost row) regrouped
    -- ids < N first, in their original order, ids >= N after, in their original order -- and per row the position of its first ghost
    entry, ptr[v + 1] where it has none (dory_row_edge_split_plan; no context, no GPU).  The copy Context.gatmh_row_gather_edge_split
    builds per adjacency."""
    lib = lib or load()
    ptr, idx = np.ascontiguousarray(ptr, np.uint64), np.ascontiguousarray(idx, np.uint32)
    if ptr.size < 1:
        raise DoryError("row_edge_split_plan: ptr is empty")
    rows = ptr.size - 1
    if rows and int(ptr[rows]) > idx.size:
        raise DoryError(f"row_edge_split_plan: ptr names {int(ptr[rows])} entries, idx has {idx.size}")
    out, mid = np.zeros(idx.size, np.uint32), np.zeros(rows, np.uint64)
    rc = lib.dory_row_edge_split_plan(_ptr(ptr), _ptr(idx), rows, int(N), _ptr(out), _ptr(mid))
    if rc != 0:
        raise DoryError(f"dory_row_edge_split_plan failed ({rc})")
    return out, mid


def gatmh_row_gather_bf16_wide_form(K, D, ld, lib=None):
    """None where a pass of the row-gather family over K heads of D features on rows of ld floats has no wide bf16 form (the narrow
    form runs), else (lanes_per_row, lanes_per_head, scores_from_row): the rule Context.gatmh_row_gather_bf16_wide applies
    (dory_gatmh_row_gather_bf16_wide_form; no context, no GPU)"""
    lib = lib or load()
    lr, lh, el = C.c_uint32(), C.c_uint32(), C.c_int32()
    if not lib.dory_gatmh_row_gather_bf16_wide_form(int(K), int(D), int(ld), C.byref(lr), C.byref(lh), C.byref(el)):
        return None
    return lr.value, lh.value, bool(el.value)


def k1_bf16_wide_form(ld, slab=0, lib=None):
    """None where K1 has no wide bf16 form for rows of ld floats under option spmm_slab = slab (the narrow form runs), else
    (lanes, chunks): the instantiation of spmm_rows_bf16x8_kernel that Context.k1_bf16_wide selects -- a row pass covers
    lanes x chunks 16-byte chunks, gridDim.y passes cover the row (dory_k1_bf16_wide_form; no context, no GPU)"""
    lib = lib or load()
    g, k = C.c_uint32(), C.c_uint32()
    if not lib.dory_k1_bf16_wide_form(int(ld), int(slab), C.byref(g), C.byref(k)):
        return None
    return g.value, k.value


class Context:
    """One GPU / one graph partition ("node" in the reference).  Thin, 1:1 with the C-ABI."""

    def __init__(self, device=0, lib=None):
        self.lib = lib or load()
        h = C.c_void_p()
        rc = self.lib.dory_create(device, C.byref(h))
        if rc != 0:
            raise DoryError(f"dory_create failed ({rc}): {self.lib.dory_last_error(None).decode()}")
        self.h = h
        self._keep = []

    def _ck(self, rc):
        if rc != 0:
            raise DoryError(f"dorylus_hip error {rc}: {self.lib.dory_last_error(self.h).decode()}")

    def close(self):
        if self.h:
            self.lib.dory_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup -----------------------------------------------------------------
    def configure(self, gnn, dims, global_vtx_cnt, node_id=0, num_nodes=1):
        d = np.ascontiguousarray(dims, dtype=np.uint32)
        self.dims = [int(x) for x in d]
        self.L = len(d) - 1
        self._ck(self.lib.dory_configure(self.h, gnn, self.L, _ptr(d), global_vtx_cnt, node_id, num_nodes))

    def graph_upload(self, g):
        """g: dict with the fields of graph.<id>.bin."""
        cp = np.ascontiguousarray(g["colPtr"], np.uint64)
        ri = np.ascontiguousarray(g["rowIdx"], np.uint32)
        cv = np.ascontiguousarray(g["cscVal"], np.float32)
        rp = np.ascontiguousarray(g["rowPtr"], np.uint64)
        ci = np.ascontiguousarray(g["colIdx"], np.uint32)
        rv = np.ascontiguousarray(g["csrVal"], np.float32)
        nm = np.ascontiguousarray(g["norm"], np.float32)
        self.N = int(g["localVtxCnt"])
        self._ck(self.lib.dory_graph_upload(
            self.h, self.N, int(g["srcGhostCnt"]), int(g["dstGhostCnt"]), int(ri.size), _ptr(cp),
            _ptr(ri), _ptr(cv), int(ci.size), _ptr(rp), _ptr(ci), _ptr(rv), _ptr(nm)))

    def gatmh_heads(self, heads):
        h = np.ascontiguousarray(heads, np.uint32)
        assert h.size == self.L
        self.heads = [int(x) for x in h]
        self._ck(self.lib.dory_gatmh_heads(self.h, _ptr(h)))

    def preallocate(self):
        self._ck(self.lib.dory_preallocate(self.h))

    # -- tensors ------------------------------------------------------------------
    def info(self, layer, name, ptr=True):
        """(rows, cols, ld, device pointer).  ptr=False asks for the shape alone (pointer None): a tensor whose raw pointer has
        been handed out is never again the target of a fused halo pack (halo_fused_pack)."""
        rows, cols, ld, p = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_void_p()
        self._ck(self.lib.dory_tensor_info(self.h, layer, name.encode(), C.byref(rows), C.byref(cols),
                                           C.byref(ld), C.byref(p) if ptr else None))
        return rows.value, cols.value, ld.value, p.value

    def upload(self, layer, name, a):
        rows, cols, _, _ = self.info(layer, name, ptr=False)
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.size != rows * cols:
            raise DoryError(f"upload {name}@{layer}: got {a.shape}, tensor is {rows}x{cols}")
        self._ck(self.lib.dory_tensor_upload(self.h, layer, name.encode(), _ptr(a)))

    def download(self, layer, name):
        rows, cols, _, _ = self.info(layer, name, ptr=False)
        a = np.empty((rows, cols), np.float32)
        self._ck(self.lib.dory_tensor_download(self.h, layer, name.encode(), _ptr(a)))
        return a

    def fill_uniform(self, layer, name, seed, lo=-1.0, hi=1.0, row_ids=None):
        ids = None if row_ids is None else np.ascontiguousarray(row_ids, np.uint32)
        self._ck(self.lib.dory_tensor_fill_uniform(self.h, layer, name.encode(), seed, lo, hi, _ptr(ids)))

    def labels_upload(self, labels):
        l = np.ascontiguousarray(labels, np.uint32)
        self._ck(self.lib.dory_labels_upload(self.h, _ptr(l)))

    # -- weights ---------------------------------------------------------------------
    def _wshape(self, layer, name):
        heads = getattr(self, "heads", None)
        if heads is not None:   # multi-head GAT extension: the last layer keeps K_out copies of the class width
            zw = self.dims[layer + 1] * (heads[layer] if layer == self.L - 1 else 1)
            return (self.dims[layer], zw) if name == "w" else (zw, 1)
        return (self.dims[layer], self.dims[layer + 1]) if name == "w" else (self.dims[layer + 1], 1)

    def weight_set(self, layer, name, w):
        w = np.ascontiguousarray(w, np.float32)
        assert w.size == int(np.prod(self._wshape(layer, name)))
        self._ck(self.lib.dory_weight_set(self.h, layer, name.encode(), _ptr(w)))

    def weight_get(self, layer, name="w"):
        w = np.empty(self._wshape(layer, name), np.float32)
        self._ck(self.lib.dory_weight_get(self.h, layer, name.encode(), _ptr(w)))
        return w

    def weight_grad_get(self, layer, name="w"):
        w = np.empty(self._wshape(layer, name), np.float32)
        self._ck(self.lib.dory_weight_grad_get(self.h, layer, name.encode(), _ptr(w)))
        return w

    def weight_grad_set(self, layer, grad, name="w"):
        g = np.ascontiguousarray(grad, np.float32)
        assert g.shape == self._wshape(layer, name)
        self._ck(self.lib.dory_weight_grad_set(self.h, layer, name.encode(), _ptr(g)))

    def weights_init_xavier(self):
        self._ck(self.lib.dory_weights_init_xavier(self.h))

    # -- hot path ------------------------------------------------------------------------
    def aggregate(self, layer, direction):
        self._ck(self.lib.dory_aggregate(self.h, layer, direction))

    def apply_vertex(self, layer, direction):
        self._ck(self.lib.dory_apply_vertex(self.h, layer, direction))

    def apply_edge(self, layer, direction):
        self._ck(self.lib.dory_apply_edge(self.h, layer, direction))

    def predict_gat(self, layer):
        self._ck(self.lib.dory_predict_gat(self.h, layer))

    def train_stat(self):
        a, l, n = C.c_float(), C.c_float(), C.c_uint32()
        self._ck(self.lib.dory_train_stat(self.h, C.byref(a), C.byref(l), C.byref(n)))
        return a.value, l.value, n.value

    def train_stat_global(self):
        """the same summed over all partitions (a collective: every rank calls it)"""
        a, l, n = C.c_float(), C.c_float(), C.c_uint32()
        self._ck(self.lib.dory_train_stat_global(self.h, C.byref(a), C.byref(l), C.byref(n)))
        return a.value, l.value, n.value

    # -- halo / comm ------------------------------------------------------------------------
    def halo_plan(self, direction, send_lists, recv_slot_lists):
        sc = np.array([len(x) for x in send_lists], np.uint32)
        rc = np.array([len(x) for x in recv_slot_lists], np.uint32)
        sl = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32) for x in send_lists] + [np.zeros(0, np.uint32)]), np.uint32)
        rs = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint32) for x in recv_slot_lists] + [np.zeros(0, np.uint32)]), np.uint32)
        self._ck(self.lib.dory_halo_plan(self.h, direction, _ptr(sc), _ptr(sl), _ptr(rc), _ptr(rs)))

    def comm_unique_id(self):
        buf = np.zeros(128, np.uint8)
        rc = self.lib.dory_comm_unique_id(_ptr(buf))
        if rc != 0:
            raise DoryError("ncclGetUniqueId failed")
        return buf

    def comm_init(self, id128, rank, nranks):
        b = np.ascontiguousarray(id128, np.uint8)
        self._ck(self.lib.dory_comm_init(self.h, _ptr(b), rank, nranks))

    @staticmethod
    def comm_init_local(ctxs):
        """in-process device transport: the contexts (rank i = ctxs[i]) of this process become each other's peers -- rows
        travel device -> device on the sender's comm stream, ordered by cross-context events (dory_comm_init_local).
        Drive each rank from its own thread afterwards (ctypes calls release the GIL)."""
        arr = (C.c_void_p * len(ctxs))(*[c.h for c in ctxs])
        rc = ctxs[0].lib.dory_comm_init_local(arr, len(ctxs))
        if rc != 0:
            msgs = [c.lib.dory_last_error(c.h).decode() for c in ctxs]
            raise DoryError(f"dory_comm_init_local failed ({rc}): " + "; ".join(m for m in msgs if m))

    def set_host_transport(self, alltoallv, allreduce):
        """alltoallv(send: np.ndarray, send_counts, send_offsets, recv: np.ndarray, recv_counts, recv_offsets) and
        allreduce(buf: np.ndarray) move host floats between the ranks (e.g. over gloo); everything else of the
        multi-rank epoch stays in the library.  (None, None) returns to RCCL."""
        if alltoallv is None:
            self._tx = None
            self._ck(self.lib.dory_comm_set_host_transport(self.h, ALLTOALLV_FN(0), ALLREDUCE_FN(0), None))
            return

        def a2a(user, send, sc, so, recv, rc, ro, P):
            try:
                scn, son = np.ctypeslib.as_array(sc, (P,)).copy(), np.ctypeslib.as_array(so, (P,)).copy()
                rcn, ron = np.ctypeslib.as_array(rc, (P,)).copy(), np.ctypeslib.as_array(ro, (P,)).copy()
                ns, nr = int((son + scn).max()), int((ron + rcn).max())
                sa = np.ctypeslib.as_array(send, (max(ns, 1),))
                ra = np.ctypeslib.as_array(recv, (max(nr, 1),))
                alltoallv(sa, scn, son, ra, rcn, ron)
                return 0
            except Exception:       # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        def ar(user, buf, n):
            try:
                allreduce(np.ctypeslib.as_array(buf, (int(n),)))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        self._tx = (ALLTOALLV_FN(a2a), ALLREDUCE_FN(ar))      # keep the thunks alive
        self._ck(self.lib.dory_comm_set_host_transport(self.h, self._tx[0], self._tx[1], None))

    # -- scatter messages: the reference's own graph-server <-> graph-server wire (include/dorylus_wire.h) -------------------
    def halo_wire_ids(self, local_to_global, src_ghost_gvids, dst_ghost_gvids):
        a = [np.ascontiguousarray(x, np.uint32) for x in (local_to_global, src_ghost_gvids, dst_ghost_gvids)]
        self._ck(self.lib.dory_halo_wire_ids(self.h, *[_ptr(x) for x in a]))

    def scatter_msgs_layout(self, layer, direction, name=None, max_msg_bytes=0):
        """([(peer, first_row, rows, offset, bytes), ...], total_bytes): the messages of that exchange inside one buffer"""
        n, total = C.c_uint32(), C.c_uint64()
        nm = name.encode() if name else None
        self._ck(self.lib.dory_scatter_msgs_layout(self.h, layer, direction, nm, int(max_msg_bytes), None, 0, C.byref(n), C.byref(total)))
        arr = (ScatterMsg * max(n.value, 1))()
        self._ck(self.lib.dory_scatter_msgs_layout(self.h, layer, direction, nm, int(max_msg_bytes), arr, n.value, C.byref(n), C.byref(total)))
        return [(m.peer, m.first_row, m.rows, m.offset, m.bytes) for m in arr[:n.value]], total.value

    def scatter_msgs_pack(self, layer, direction, dev_ptr, name=None, max_msg_bytes=0):
        self._ck(self.lib.dory_scatter_msgs_pack(self.h, layer, direction, name.encode() if name else None, int(max_msg_bytes), C.c_void_p(dev_ptr)))

    def scatter_msgs_deliver(self, msgs, name=None):
        """msgs: whole messages (bytes, or contiguous uint8 arrays), from any senders in any order"""
        keep = [np.frombuffer(m, np.uint8) if isinstance(m, (bytes, bytearray, memoryview)) else np.ascontiguousarray(m, np.uint8) for m in msgs]
        ptrs = (C.c_void_p * max(len(keep), 1))(*[k.ctypes.data for k in keep])
        sizes = (C.c_uint64 * max(len(keep), 1))(*[k.size for k in keep])
        self._ck(self.lib.dory_scatter_msgs_deliver(self.h, name.encode() if name else None, ptrs, sizes, len(keep)))

    def scatter_msgs_unpack(self, layer, direction, dev_ptr, count, name=None):
        """`count` records (id, cols floats) that are in device memory already"""
        self._ck(self.lib.dory_scatter_msgs_unpack(self.h, layer, direction, name.encode() if name else None, C.c_void_p(dev_ptr), int(count)))

    def scatter_msgs_finish(self, layer, direction, name=None, check=True):
        """(rows written, unknown ids, duplicates) of the round that ends; check=False: (return code, rows, unknown, duplicates)"""
        r, u, d = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.lib.dory_scatter_msgs_finish(self.h, layer, direction, name.encode() if name else None, C.byref(r), C.byref(u), C.byref(d))
        if not check:
            return rc, r.value, u.value, d.value
        self._ck(rc)
        return r.value, u.value, d.value

    def set_scatter_transport(self, exchange, allreduce, max_msg_bytes=0):
        """exchange(msgs: [(peer, uint8 array), ...]) sends this rank's messages and, before it returns, hands every message that
        arrived for this rank to scatter_msgs_deliver (e.g. over gloo, as bytes); allreduce(buf) as set_host_transport's.
        (None, None) returns to RCCL."""
        if exchange is None:
            self._tx = None
            self._ck(self.lib.dory_comm_set_scatter_transport(self.h, SCATTER_EXCHANGE_FN(0), ALLREDUCE_FN(0), None, 0))
            return

        def ex(user, ctx, host_buf, msgs, n):
            try:
                out = []
                for i in range(n):
                    m = msgs[i]
                    out.append((int(m.peer), np.ctypeslib.as_array(C.cast(host_buf + m.offset, C.POINTER(C.c_uint8)), (int(m.bytes),))))
                exchange(out)
                return 0
            except Exception:       # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1

        def ar(user, buf, n):
            try:
                allreduce(np.ctypeslib.as_array(buf, (int(n),)))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        self._tx = (SCATTER_EXCHANGE_FN(ex), ALLREDUCE_FN(ar))      # keep the thunks alive
        self._ck(self.lib.dory_comm_set_scatter_transport(self.h, self._tx[0], self._tx[1], None, int(max_msg_bytes)))

    def halo_exchange(self, layer, direction):
        self._ck(self.lib.dory_halo_exchange(self.h, layer, direction))

    def halo_pack(self, layer, direction, dev_ptr):
        self._ck(self.lib.dory_halo_pack(self.h, layer, direction, C.c_void_p(dev_ptr)))

    def halo_unpack(self, layer, direction, dev_ptr):
        self._ck(self.lib.dory_halo_unpack(self.h, layer, direction, C.c_void_p(dev_ptr)))

    def halo_pack_tensor(self, layer, name, direction, dev_ptr):
        self._ck(self.lib.dory_halo_pack_tensor(self.h, layer, name.encode(), direction, C.c_void_p(dev_ptr)))

    def halo_unpack_tensor(self, layer, name, direction, dev_ptr):
        self._ck(self.lib.dory_halo_unpack_tensor(self.h, layer, name.encode(), direction, C.c_void_p(dev_ptr)))

    def _switch(self, fn, value):       # a feature switch's setter dory_<name>(ctx, int) (the table: switch_specs())
        self._ck(fn(self.h, int(value)))

    def _stats(self, fn, n, names=None):        # the n values of a dory_<name>_stats entry point: a tuple, or with names a dict
        v = [C.c_uint64(0) for _ in range(n)]
        self._ck(fn(self.h, *[C.byref(x) for x in v]))
        v = tuple(int(x.value) for x in v)
        return dict(zip(names, v)) if names else v

    def halo_fused_pack(self, on=True):
        """the GEMM epilogues write the send rows of the exchange that follows (opt-in; dory_halo_fused_pack)"""
        self._switch(self.lib.dory_halo_fused_pack, on)

    def gat_bf16_gather(self, mode, wide=False):
        """GAT prototype: the aggregations gather their rows rounded to bf16 (opt-in; dory_gat_bf16_gather) -- mode 1: those that
        read z / fg_z, 2: the backward's A^T grad too; wide: 16-byte gathers on K1s for rows of 128 floats or more, same bits"""
        self._ck(self.lib.dory_gat_bf16_gather(self.h, int(mode), int(wide)))

    def gat_bf16_gather_stats(self):
        """aggregations that ran on bf16 rows per kernel family: dict(k1s, k1s_wide, k1, fp32_fallbacks)"""
        v = [C.c_uint64(0) for _ in range(4)]
        self._ck(self.lib.dory_gat_bf16_gather_stats(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("k1s", "k1s_wide", "k1", "fp32_fallbacks"), (int(x.value) for x in v)))

    def halo_bf16_rows(self, on=True):
        """exchanges whose consumer gathers bf16 rows ship bf16 rows (opt-in; dory_halo_bf16_rows): half the bytes, the same bits"""
        self._switch(self.lib.dory_halo_bf16_rows, on)

    def halo_bf16_rows_stats(self):
        """(packs that wrote bf16 rows, their bytes, packs that wrote fp32 rows while the switch was on)"""
        return self._stats(self.lib.dory_halo_bf16_rows_stats, 3)

    GHOST_STATES = ("FP32", "TWIN", "BOTH")     # DORY_GHOST_FP32 / _TWIN / _BOTH

    def halo_bf16_ghosts(self, on=True):
        """bf16 halo rows stay bf16 on arrival, in a bf16 twin of the ghost tensor that the aggregation on bf16 rows gathers from
        (opt-in on top of halo_bf16_rows; dory_halo_bf16_ghosts; after preallocate)"""
        self._switch(self.lib.dory_halo_bf16_ghosts, on)

    def halo_bf16_ghosts_stats(self):
        """dict(landed_direct, landed_by_kernel, conversions_skipped, widened, twin_bytes)"""
        return self._stats(self.lib.dory_halo_bf16_ghosts_stats, 5, ("landed_direct", "landed_by_kernel", "conversions_skipped", "widened", "twin_bytes"))

    def halo_bf16_ghost_peek(self, layer, name):
        """(device pointer of the tensor's bf16 twin or None, state "FP32" / "TWIN" / "BOTH"): which copy holds the current rows"""
        p, st = C.c_void_p(), C.c_int(0)
        self._ck(self.lib.dory_halo_bf16_ghost_peek(self.h, layer, name.encode(), C.byref(p), C.byref(st)))
        return p.value, self.GHOST_STATES[st.value]

    def halo_wire_row(self, layer, direction):
        """(bytes per element, elements per row) of what halo_exchange / halo_pack of (layer, direction) put on the wire now"""
        e, n = C.c_uint32(), C.c_uint32()
        self._ck(self.lib.dory_halo_wire_row(self.h, layer, direction, C.byref(e), C.byref(n)))
        return e.value, n.value

    def halo_fused_pack_stats(self):
        """(exchanges that skipped their pack kernel, the send rows of those, exchanges that packed although the feature was on)"""
        return self._stats(self.lib.dory_halo_fused_pack_stats, 3)

    def halo_fused_pack_bf16(self, on=True):
        """the fused halo pack also serves exchanges that ship bf16 rows: the GEMM epilogues round and write them (opt-in on top of
        halo_fused_pack and halo_bf16_rows; dory_halo_fused_pack_bf16)"""
        self._switch(self.lib.dory_halo_fused_pack_bf16, on)

    def halo_fused_pack_bf16_stats(self):
        """(exchanges whose bf16 send rows a GEMM epilogue wrote, the send rows of those)"""
        return self._stats(self.lib.dory_halo_fused_pack_bf16_stats, 2)

    def halo_fused_pack_rowwise(self, on=True):
        """the fused halo pack also serves exchanges whose source a row-wise kernel writes (g, h of a transform-first layer, the GAT
        prototype's last-layer grad): the send forms of those kernels write the rows (opt-in on top of halo_fused_pack, and of
        halo_fused_pack_bf16 for bf16 rows; dory_halo_fused_pack_rowwise)"""
        self._switch(self.lib.dory_halo_fused_pack_rowwise, on)

    def halo_fused_pack_rowwise_stats(self):
        """(exchanges whose send rows a row-wise producer wrote, the send rows of those)"""
        return self._stats(self.lib.dory_halo_fused_pack_rowwise_stats, 2)

    def gatmh_bwd_merged_exchange(self, on=True):
        """the multi-head GAT's backward sweep ships do and st of a sent vertex as ONE merged row [do | st] in one exchange instead of
        two (opt-in; dory_gatmh_bwd_merged_exchange); with halo_fused_pack on and the sweep forms running, the row-wise kernel that
        produces st writes the send rows itself and no pack kernel runs.  All ranks must set the same value"""
        self._switch(self.lib.dory_gatmh_bwd_merged_exchange, on)

    def gatmh_bwd_merged_exchange_stats(self):
        """(merged exchanges made, their send rows, those of them whose rows the producer wrote, backward passes that kept the two
        exchanges although the switch was on)"""
        return self._stats(self.lib.dory_gatmh_bwd_merged_exchange_stats, 4)

    def gatmh_bwd_wire_row(self, layer):
        """(floats per merged row, of which do, of which st) of the tensors' layer `layer`, as the wire stands now"""
        r, d, s = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(self.lib.dory_gatmh_bwd_wire_row(self.h, layer, C.byref(r), C.byref(d), C.byref(s)))
        return r.value, d.value, s.value

    def gatmh_halo_bf16(self, on=True):
        """the 8-head GAT under the rule of halo_bf16_rows (opt-in, on top of it; dory_gatmh_halo_bf16): z ships bf16 while
        gatmh_bf16_gather >= 1, the backward sweep's do while it is 2; st stays fp32"""
        self._switch(self.lib.dory_gatmh_halo_bf16, on)

    def gatmh_halo_bf16_stats(self):
        """(fwd_bf16_exchanges, bwd_bf16_exchanges, bwd_bf16_rows, producer_packed_bf16) of the eager exchanges since dory_create"""
        return self._stats(self.lib.dory_gatmh_halo_bf16_stats, 4)

    def gatmh_bwd_wire_do(self, layer):
        """(elem_bytes, elems) of the do part of the backward rows of `layer` as the wire stands now"""
        e, n = C.c_uint32(), C.c_uint32()
        self._ck(self.lib.dory_gatmh_bwd_wire_do(self.h, layer, C.byref(e), C.byref(n)))
        return int(e.value), int(n.value)

    def gatmh_bwd_pack(self, layer, dev_ptr):
        """the backward plan's send rows of do / st of `layer` as merged rows into a device buffer (option gatmh_bwd_phase = 1 / 2:
        the caller moves them)"""
        self._ck(self.lib.dory_gatmh_bwd_pack(self.h, layer, C.c_void_p(dev_ptr)))

    def gatmh_bwd_unpack(self, layer, dev_ptr):
        """received merged rows out of a device buffer into bg_do / bg_st of `layer`, whole ghost rows (padding zeroed)"""
        self._ck(self.lib.dory_gatmh_bwd_unpack(self.h, layer, C.c_void_p(dev_ptr)))

    def gatmh_row_gather(self, mode=1):
        """the multi-head GAT's row-gather kernels with ghost rows (dory_gatmh_row_gather): 0 (default) = where a partitioned
        aggregate would otherwise be refused (no sweep layout, no blocked layout, a head shape neither covers), 1 = in place of
        every other family, single partitions included (tests, measurement)"""
        self._switch(self.lib.dory_gatmh_row_gather, mode)

    def gatmh_row_gather_stats(self):
        """(fwd, dst_edge_pass, dst_rowwise, src): the passes the row-gather family ran since dory_create, eager calls and recordings"""
        return self._stats(self.lib.dory_gatmh_row_gather_stats, 4)

    def gatmh_row_gather_bf16(self, on=1):
        """option gatmh_bf16_gather reaches the row-gather family (dory_gatmh_row_gather_bf16): 0 (default) = refused there as ever,
        1 = where the dispatch selects the family its bf16 forms run (8-byte gathers from the shadow rows, fp32 arithmetic)"""
        self._switch(self.lib.dory_gatmh_row_gather_bf16, on)

    def gatmh_row_gather_bf16_stats(self):
        """(fwd, dst_edge_pass, src): the passes of the row-gather family that ran a bf16 form since dory_create"""
        return self._stats(self.lib.dory_gatmh_row_gather_bf16_stats, 3)

    GATMH_BF16_GHOSTS_STATS = ("fwd_kept", "bwd_kept", "bwd_kept_merged", "twin_reads_rows", "twin_reads_sweep", "scores_from_twin", "widened")

    def gatmh_bf16_ghosts(self, on=True):
        """fg_z and bg_do of the multi-head GAT get bf16 twins too (dory_gatmh_bf16_ghosts; opt-in on top of halo_bf16_ghosts, after
        preallocate): rows that travel as bf16 (halo_bf16_rows + gatmh_halo_bf16 + option gatmh_bf16_gather) stay bf16 where the bf16
        edge passes gather them; dory_apply_edge forms fg_el / fg_er from the twin"""
        self._switch(self.lib.dory_gatmh_bf16_ghosts, on)

    def gatmh_bf16_ghosts_stats(self):
        """dict of the eager calls since dory_create: fwd_kept / bwd_kept / bwd_kept_merged (exchanges and unpacks whose rows stayed in
        fg_z's / bg_do's twin, bg_do's through a merged row), twin_reads_rows / twin_reads_sweep (bf16 passes of the row-gather family /
        the sweep forms that read a twin instead of converting ghost rows), scores_from_twin (dory_apply_edge), widened (for a reader
        of fp32 rows)"""
        return self._stats(self.lib.dory_gatmh_bf16_ghosts_stats, 7, self.GATMH_BF16_GHOSTS_STATS)

    GATMH_HUB_SPLIT_STATS = ("fwd", "dst_edge_pass", "src", "in_hub_rows", "in_chunks", "out_hub_rows", "out_chunks")

    def gatmh_row_gather_hub_split(self, chunk_entries):
        """hub rows of the row-gather family run as chunks (dory_gatmh_row_gather_hub_split): 0 (default) = off; else a multiple of 64
        in 64..2^20 -- a row with more adjacency entries than that is cut into consecutive chunks of that many, each on a lane group
        of its own, and merged in chunk order (no atomics: same input, same bits); rows that are not cut keep their bits"""
        self._ck(self.lib.dory_gatmh_row_gather_hub_split(self.h, int(chunk_entries)))

    def gatmh_row_gather_hub_split_stats(self):
        """dict: fwd / dst_edge_pass / src (passes that ran split since dory_create), in_hub_rows / in_chunks / out_hub_rows /
        out_chunks (the current chunk plans of the in-edges and the out-edges)"""
        return self._stats(self.lib.dory_gatmh_row_gather_hub_split_stats, 7, self.GATMH_HUB_SPLIT_STATS)

    GATMH_ROWS_OVERLAP_STATS = ("fwd_split", "src_split", "fwd_in_flight", "src_in_flight", "in_interior_rows", "out_interior_rows",
                                "bwd_deferred")

    def gatmh_row_gather_overlap(self, on=1):
        """the row-gather family runs its interior rows beside the exchange (dory_gatmh_row_gather_overlap): 0 (default) = off; 1 = where
        an adjacency has interior rows (every entry local: row_interior_plan) and others, the forward and the backward's source side
        launch the interior rows first -- beside the exchange in flight, if any -- then wait for the ghost rows and launch the rest;
        every row is computed whole by the same kernel body, so every bit stays"""
        self._ck(self.lib.dory_gatmh_row_gather_overlap(self.h, int(on)))

    def gatmh_row_gather_overlap_stats(self):
        """dict: fwd_split / src_split (passes that ran as two launches since dory_create), fwd_in_flight / src_in_flight (those of
        them with an exchange in flight beside the first), in_interior_rows / out_interior_rows (the current plans of the in-edges
        and the out-edges), bwd_deferred (backward exchanges issued deferred)"""
        return self._stats(self.lib.dory_gatmh_row_gather_overlap_stats, 7, self.GATMH_ROWS_OVERLAP_STATS)

    GATMH_ROWS_EDGE_SPLIT_STATS = ("fwd_split", "src_split", "fwd_in_flight", "src_in_flight", "in_local_entries", "out_local_entries",
                                   "hub_fallbacks", "wide_not_taken")

    def gatmh_row_gather_edge_split(self, value=1):
        """the row-gather family walks every row's local entries before its ghost entries (dory_gatmh_row_gather_edge_split): 0 (default)
        = off; 1 = the forward and the backward's source side run the carry kernels over a local-first copy of the ids
        (row_edge_split_plan) -- with an exchange in flight the local entries and the self edge first, beside it, the state of the
        boundary rows parked, then the wait and the ghost entries; with nothing in flight one launch; 2 = always the two launches.
        The same bits either way; against 0 only m keeps its bits (other association of the sums)"""
        self._ck(self.lib.dory_gatmh_row_gather_edge_split(self.h, int(value)))

    def gatmh_row_gather_edge_split_stats(self):
        """dict: fwd_split / src_split (passes that ran the carry kernels since dory_create), fwd_in_flight / src_in_flight (those of
        them with an exchange in flight beside the first launch), in_local_entries / out_local_entries (the current copies of the
        in-edges and the out-edges), hub_fallbacks (passes left to the hub chunk plan), wide_not_taken (bf16 passes that ran the
        narrow carry kernel with gatmh_row_gather_bf16_wide on)"""
        return self._stats(self.lib.dory_gatmh_row_gather_edge_split_stats, 8, self.GATMH_ROWS_EDGE_SPLIT_STATS)

    GATMH_ROWS_BF16_WIDE_STATS = ("fwd", "dst_edge_pass", "src", "narrow_while_on")

    def gatmh_row_gather_bf16_wide(self, on=1):
        """the row-gather family's bf16 passes gather 16 bytes a lane (dory_gatmh_row_gather_bf16_wide): 0 (default) = off; 1 = where
        gatmh_row_gather_bf16_wide_form has a form for the shape, a bf16 pass keeps eight features a lane on half the lanes per row --
        the narrow bf16 form's bits in every tensor; inert while gatmh_row_gather_bf16 is off"""
        self._ck(self.lib.dory_gatmh_row_gather_bf16_wide(self.h, int(on)))

    def gatmh_row_gather_bf16_wide_stats(self):
        """dict: fwd / dst_edge_pass / src (passes that ran the wide form since dory_create: eager calls and recordings),
        narrow_while_on (bf16 passes of the family that ran narrow with the switch on)"""
        return self._stats(self.lib.dory_gatmh_row_gather_bf16_wide_stats, 4, self.GATMH_ROWS_BF16_WIDE_STATS)

    K1_BF16_WIDE_STATS = ("wide", "narrow_while_on")

    def k1_bf16_wide(self, on=1):
        """K1's aggregations on bf16 rows gather 16 bytes a lane (dory_k1_bf16_wide; GCN and the GAT prototype): 0 (default) = off;
        1 = where k1_bf16_wide_form has a form for the row and slab width, every launch of the aggregation keeps eight features a lane
        and chunk -- the narrow bf16 form's bits in every tensor; inert while no bf16 gather mode is on"""
        self._ck(self.lib.dory_k1_bf16_wide(self.h, int(on)))

    def k1_bf16_wide_stats(self):
        """dict: wide (aggregations K1 ran in the wide form since dory_create: eager calls and recordings), narrow_while_on
        (aggregations on bf16 rows K1 ran narrow with the switch on)"""
        return self._stats(self.lib.dory_k1_bf16_wide_stats, 2, self.K1_BF16_WIDE_STATS)

    # -- optimiser ---------------------------------------------------------------------------
    def adam_config(self, lr):
        self._ck(self.lib.dory_adam_config(self.h, lr))

    def weight_update(self, layer):
        self._ck(self.lib.dory_weight_update(self.h, layer))

    # -- misc -----------------------------------------------------------------------------------
    def sync(self):
        self._ck(self.lib.dory_sync(self.h))

    def debug_occupy_cus(self, workgroups, usec):
        self._ck(self.lib.dory_debug_occupy_cus(self.h, workgroups, usec))

    def set_streams(self, compute=None, comm=None):
        self._ck(self.lib.dory_set_streams(self.h, C.c_void_p(compute or 0), C.c_void_p(comm or 0)))

    def timing_enable(self, on=True):
        self._ck(self.lib.dory_timing_enable(self.h, int(on)))

    def timing_get(self, family):
        ms, n = C.c_double(), C.c_uint64()
        self._ck(self.lib.dory_timing_get(self.h, family.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_reset(self):
        self._ck(self.lib.dory_timing_reset(self.h))

    def set_option(self, key, value):
        self._ck(self.lib.dory_set_option(self.h, key.encode(), int(value)))

    def transform_first_active(self):
        return bool(self.lib.dory_transform_first_active(self.h))

    def transform_first_layer(self, layer):
        return bool(self.lib.dory_transform_first_layer(self.h, int(layer)))

    def get_option(self, key):
        v = C.c_int64(0)
        self._ck(self.lib.dory_get_option(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    # epoch graph (hipGraph replay of one recorded epoch; single partition)
    def epoch_graph_begin(self):
        self._ck(self.lib.dory_epoch_graph_begin(self.h))

    def epoch_graph_end(self):
        self._ck(self.lib.dory_epoch_graph_end(self.h))

    def epoch_graph_launch(self, epochs=1):
        self._ck(self.lib.dory_epoch_graph_launch(self.h, int(epochs)))

    def epoch_graph_drop(self):
        self._ck(self.lib.dory_epoch_graph_drop(self.h))
