"""dory_halo_bf16_rows (include/dorylus_hip.h) in numpy: the rounding of an fp32 to bf16 (nearest, ties to even, on the bits), the
layout of a packed halo buffer whose rows hold `row_elems` bf16 values (padded: the tensor's ld; exact: cols rounded up to a
multiple of 4, zeros behind cols), the unpack that writes a whole ld-wide ghost row (widened values, then zeros), the rule that
says which exchange ships bf16, and the generator of the bit patterns that tests/test_halo_bf16_reference.py compares against
torch on the CPU and tests/test_gpu_halo_bf16_rows.py feeds the kernels."""
import numpy as np

from halo_exact_ref import pad_ld


def round_bits(x):
    """fp32 values (any shape) -> their bf16 bits as uint16: (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bits.  Not for
    NaN (a NaN with a small payload would carry into infinity; the hardware keeps it a NaN)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(b):
    """bf16 bits (uint16) -> the fp32 with the same value: bits << 16"""
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def rounded(x):
    """fp32 values as a consumer that gathers bf16 rows sees them"""
    return widen(round_bits(x))


def row_elems(cols, exact):
    """elements of a packed row: ld (one-column tensors, ld == 1: 4), or with halo_exact_rows cols rounded up to a multiple of 4"""
    return ((cols if exact else pad_ld(cols)) + 3) & ~3


def pack(x, rows, cols, exact):
    """x: (N, >= cols) rows of a tensor; rows: the send list (may repeat).  Returns the packed buffer as uint16: len(rows) x
    row_elems bf16, zeros in [cols, row_elems) (the owner's zero padding in the padded form, written by the pack in the exact one)"""
    rows = np.asarray(rows, np.int64)
    out = np.zeros((rows.size, row_elems(cols, exact)), np.uint16)
    out[:, :cols] = round_bits(np.ascontiguousarray(x[rows, :cols], np.float32))
    return out.reshape(-1)


def unpack(ghost_raw, slots, buf, cols, exact):
    """ghost_raw: (G, ld) raw rows of a ghost tensor, changed in place: row slots[i] = widened buf row i in [0, row_elems), zeros
    behind -- [cols, ld) ends up zero whatever it held (the stream carries zeros in [cols, row_elems))"""
    slots = np.asarray(slots, np.int64)
    re = row_elems(cols, exact)
    ld = ghost_raw.shape[1]
    w = widen(np.asarray(buf, np.uint16).reshape(slots.size, re))
    ghost_raw[slots, :] = 0.0
    ghost_raw[slots, :min(re, ld)] = w[:, :min(re, ld)]
    return ghost_raw


def peer_offsets(counts, cols, exact):
    """(counts, offsets) of every peer's segment as the host transport's callback is given them -- in floats: rows x row_elems / 2"""
    counts = np.asarray(counts, np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    h = np.uint64(row_elems(cols, exact) // 2)
    return counts * h, off * h


GCN, GAT, GATMH = 0, 1, 2
FORWARD, BACKWARD = 0, 1


def ships_bf16(gnn, direction, gather_mode, switch=1):
    """the rule (halo_ships_bf16, csrc/abi_comm.hip): with the switch on, an exchange ships bf16 iff the aggregation that reads its
    ghost tensor gathers bf16 rows -- forward: gather mode >= 1, backward: gather mode == 2, the multi-head GAT never"""
    if not switch or gnn == GATMH:
        return False
    return gather_mode >= (1 if direction == FORWARD else 2)


NAMED = {
    "tie_down_to_even": 0x3F808000,      # 1.00390625: halfway between 0x3F80 and 0x3F81 -> 0x3F80
    "tie_up_to_even": 0x3F818000,        # halfway between 0x3F81 and 0x3F82 -> 0x3F82
    "denormal_min": 0x00000001,
    "denormal_mid": 0x00008000,          # a tie between 0 and the smallest bf16 denormal -> 0
    "denormal_big": 0x007FFFFF,          # rounds up into the smallest normal
    "plus_zero": 0x00000000,
    "minus_zero": 0x80000000,
    "flt_max": 0x7F7FFFFF,               # -> +inf
    "minus_flt_max": 0xFF7FFFFF,         # -> -inf
    "plus_inf": 0x7F800000,
    "minus_inf": 0xFF800000,
}


def named_patterns():
    """the named cases, the ties' neighbours one ulp either side, and the negative of each"""
    base = list(NAMED.values()) + [NAMED["tie_down_to_even"] + d for d in (-1, 1)] + [NAMED["tie_up_to_even"] + d for d in (-1, 1)]
    base += [0x00007FFF, 0x00008001, 0x00018000, 0x80008000, 0x807FFFFF]
    u = np.array(base, np.uint32)
    return np.unique(np.concatenate([u, u ^ np.uint32(0x80000000)]))


def patterns(n, seed=0, finite=False):
    """n fp32 values: the named patterns first (as many as fit), then random bit patterns without NaN; finite: none whose
    magnitude is infinite either (inputs of an epoch)"""
    rng = np.random.default_rng([19, seed, n])
    u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    named = named_patterns()
    k = min(n, named.size)
    u[:k] = named[:k]
    expo = (u >> 23) & 0xFF
    bad = expo == 0xFF
    if not finite:
        bad &= (u & 0x7FFFFF) != 0
    u[bad] &= np.uint32(0xBFFFFFFF)      # clear one exponent bit: a finite number with the same mantissa
    return u.view(np.float32)


def local_values(n_rows, cols, salt=0):
    """(n_rows, cols) source rows for the GPU tests: bit patterns without NaN, the named cases among them"""
    return patterns(n_rows * cols, seed=1000 * salt + cols).reshape(n_rows, cols).copy()


def wire_values(n, cols, exact):
    """a received buffer of n rows as uint16: any bf16 without NaN in [0, cols), zeros in [cols, row_elems)"""
    re = row_elems(cols, exact)
    b = round_bits(patterns(n * cols, seed=77 + cols, finite=True)).reshape(n, cols)
    out = np.zeros((n, re), np.uint16)
    out[:, :cols] = b
    return out.reshape(-1)
