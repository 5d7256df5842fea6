"""Option halo_exact_rows (include/dorylus_hip.h) in numpy: the layout of a packed halo buffer whose rows hold exactly `cols`
floats, the unpack that writes a whole ghost row (values, then zeros into the padding), the per-peer float offsets, the
mirror of the share of rows one workgroup of the exact kernels takes (csrc/elementwise.hip), and the case list that
tests/test_gpu_halo_exact_rows.py runs (tests/test_halo_exact_reference.py asserts what the list reaches, without a GPU).
Reference: Engine::verticesPushOut ships featDim floats per row (engine/utils.cpp:623-650)."""
import numpy as np


def pad_ld(cols):
    """leading dimension of a device tensor (csrc/ctx.hpp)"""
    return cols if cols <= 1 else (cols + 31) & ~31


def pack(x, rows, cols):
    """x: (N, >= cols) rows of a tensor (dense or raw ld-wide); rows: the send list (may repeat).  Row i of the buffer sits at
    float offset i * cols: one dense stream of len(rows) * cols floats"""
    rows = np.asarray(rows, np.int64)
    return np.ascontiguousarray(x[rows, :cols], np.float32).reshape(-1)


def pack_padded(x, rows, cols):
    """the same rows as option 0 ships them: ld floats each, the owner's zero padding included"""
    rows = np.asarray(rows, np.int64)
    out = np.zeros((rows.size, pad_ld(cols)), np.float32)
    out[:, :cols] = x[rows, :cols]
    return out.reshape(-1)


def unpack(ghost_raw, slots, buf, cols):
    """ghost_raw: (G, ld) raw rows of a ghost tensor, changed in place: row slots[i] = buf[i * cols : (i + 1) * cols], then
    zeros in [cols, ld) -- what the padded form leaves there, whatever the padding held before"""
    slots = np.asarray(slots, np.int64)
    ghost_raw[slots, :cols] = np.asarray(buf, np.float32).reshape(slots.size, cols)
    ghost_raw[slots, cols:] = 0.0
    return ghost_raw


def peer_offsets(counts, cols):
    """(counts, offsets) in floats of every peer's segment of a packed buffer: rows x cols, row offset x cols"""
    counts = np.asarray(counts, np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    return counts * np.uint64(cols), off * np.uint64(cols)


def rows_per_workgroup(cols):
    """rows one workgroup of gather_rows_exact_kernel / scatter_rows_exact_kernel takes: a multiple of 4 (its part of the
    stream starts on a 16-byte boundary) with about 4096 floats"""
    return ((4096 + cols - 1) // cols + 3) & ~3


def takes_exact_kernels(cols):
    """widths the new kernels move; multiples of 4 keep gather_rows_kernel / scatter_rows_kernel with the exact width"""
    return cols % 4 != 0


N_LOCAL = 64          # local vertices of every case's partition: send lists longer than this repeat rows
COLS = (1, 3, 5, 6, 20, 25, 32, 33, 41, 63, 602)
ROWS = (0, 1, 2, 3, 4, 7, 257, 5003)
# per width: the ghost counts (= rows unpacked; one context each); every case packs all of ROWS as send counts
RECV_ROWS = {
    1: (0, 1, 2, 3, 5003),
    3: (1, 2, 3, 4),
    5: (1, 2, 3, 4),
    6: (1, 3),
    20: (7,),
    25: (1, 2, 3, 4, 257),
    32: (7,),
    33: (3,),
    41: (0, 1, 2, 3, 4, 257, 5003),
    63: (2,),
    602: (1, 7, 257),
}
CASES = [(cols, nr) for cols in COLS for nr in RECV_ROWS[cols]]     # (cols, recv rows)


def send_list(n, seed):
    """n local rows in [0, N_LOCAL): a vertex goes to several peers, so rows repeat (always, once n > N_LOCAL)"""
    rng = np.random.default_rng([41, seed, n])
    rows = rng.integers(0, N_LOCAL, n).astype(np.uint32)
    if n >= 2:
        rows[n - 1] = rows[0]           # at least one repeat
    return rows


def recv_slots(n, seed):
    """a permutation of the n ghost slots"""
    return np.random.default_rng([43, seed, n]).permutation(n).astype(np.uint32)


def graph_name(n_ghosts):
    """aggregate_ref.graph name of a partition with N_LOCAL local rows and n_ghosts ghost rows on both sides"""
    e = 50 if n_ghosts else 0
    return f"ghosts:{N_LOCAL}:{n_ghosts}:{n_ghosts}:200:{e}:{e}"


def local_values(cols, salt=0):
    """distinct fp32 values (exact integers) for the N_LOCAL x cols rows of a source tensor"""
    return (np.arange(N_LOCAL * cols, dtype=np.float32).reshape(N_LOCAL, cols) + 1.0 + 100000.0 * salt)


def wire_values(n, cols):
    """distinct values for a received buffer of n rows (integers below 2^24, apart from local_values)"""
    return np.arange(n * cols, dtype=np.float32) + 5000000.0
