"""dory_halo_bf16_ghosts (include/dorylus_hip.h) in numpy, on top of tests/halo_bf16_ref.py: the keep form of the unpack -- the
received bf16 rows (row_elems a row) copied into the rows of a bf16 twin that a slot list names, at stride ld, zeros in
[row_elems, ld) -- and the widening of a whole twin into fp32 rows (bits << 16).  tests/test_halo_bf16_ghost_reference.py holds both
against torch's bf16 on the CPU and against the identity keep == round(unpack into fp32); tests/test_gpu_halo_bf16_ghosts.py holds
the kernels against them."""
import numpy as np

import halo_bf16_ref as hb

FP32, TWIN, BOTH = "FP32", "TWIN", "BOTH"      # the states dory_halo_bf16_ghost_peek reports


def keep(twin, slots, buf, cols, exact):
    """twin: (G, ld) uint16, changed in place and returned: row slots[i] = wire row i in [0, row_elems), zeros in [row_elems, ld)
    whatever it held.  buf: the received stream as uint16, len(slots) x row_elems (zeros in [cols, row_elems): the pack wrote them)"""
    slots = np.asarray(slots, np.int64)
    re = hb.row_elems(cols, exact)
    ld = twin.shape[1]
    assert twin.dtype == np.uint16 and re <= ld and ld % 32 == 0
    rows = np.asarray(buf, np.uint16).reshape(slots.size, re)
    twin[slots, :] = 0
    twin[slots, :re] = rows
    return twin


def widen(twin):
    """a whole twin (uint16, any shape) -> the fp32 rows with the same values: u16 << 16, every element"""
    return (np.asarray(twin, np.uint16).astype(np.uint32) << 16).view(np.float32)


def lands_directly(direct_plan, cols, exact):
    """an exchange of bf16 rows lands in the twin itself iff the plan is direct and a wire row is a twin row"""
    return bool(direct_plan) and hb.row_elems(cols, exact) == hb.pad_ld(cols)


def wire_bf16(gnn, direction, gather_mode, rows_switch, ghosts_switch, direct_plan, cols, scatter=False):
    """what an exchange ships (wire_bf16, csrc/abi_comm.hip): the rule of dory_halo_bf16_rows, never on the scatter transport, and
    under a direct plan only with dory_halo_bf16_ghosts on and a tensor of ld >= 4"""
    if scatter or not hb.ships_bf16(gnn, direction, gather_mode, rows_switch):
        return False
    return not direct_plan or (bool(ghosts_switch) and hb.pad_ld(cols) >= 4)
