"""dory_gatmh_bf16_ghosts (include/dorylus_hip.h) in numpy: the keep form of the merged unpack.  A received merged row of
dory_gatmh_halo_bf16 is [ do[v, 0:w) as bf16 | st[v, 0:4K) as fp32 ] (tests/gatmh_halo_bf16_ref.py); with the switch on the do part stays
bf16 in the row of bg_do's bf16 twin that the slot list names -- zeros in [w, ld), whatever the twin held -- and the st part goes into
the whole fp32 row of bg_st as before.  tests/test_gatmh_bf16_ghost_reference.py holds this against gatmh_halo_bf16_ref.unpack followed
by a rounding of the do part; tests/test_gpu_gatmh_bf16_ghosts.py holds scatter_rows_pair_bf16_keep_kernel against it."""
import numpy as np


def unpack_keep(buf, K, w, recv_lists, G, ld, ld_st, twin=None, bg_st=None):
    """the received rows (peer order, then the peer's order) into ghost slots recv_lists[peer][k].  Returns (twin [G, ld] uint16, bg_st
    [G, ld_st] float32); rows no list names keep what the given arrays hold (0x7FC1 / NaN where none is given)"""
    slots = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in recv_lists]) if len(recv_lists) else np.zeros(0, np.int64)
    assert w % 8 == 0 and w <= ld and ld % 8 == 0 and 4 * K <= ld_st
    R = w // 2 + 4 * K
    rows = np.ascontiguousarray(np.asarray(buf, np.float32).reshape(-1)[:slots.size * R]).view(np.uint8).reshape(slots.size, R * 4)
    twin = np.full((G, ld), 0x7FC1, np.uint16) if twin is None else np.array(twin, np.uint16)
    bg_st = np.full((G, ld_st), np.nan, np.float32) if bg_st is None else np.array(bg_st, np.float32)
    twin[slots] = 0
    bg_st[slots] = 0
    twin[slots, :w] = np.ascontiguousarray(rows[:, :2 * w]).view(np.uint16)
    bg_st[slots, :4 * K] = np.ascontiguousarray(rows[:, 2 * w:]).view(np.float32)
    return twin, bg_st
