"""Test-side restatement of the merged wire row of dory_gatmh_halo_bf16 (include/dorylus_hip.h): with the switch, dory_halo_bf16_rows
and gatmh_bf16_gather = 2 a sent local vertex v of a multi-head GAT layer travels as ONE row
    [ do[v, 0:w) as bf16 | st[v, 0:4K) as fp32 ]        w / 2 + 4K floats
with w = ld of do, or with halo_exact_rows its cols rounded up to a multiple of 8 (zeros behind cols): the st records start on a
16-byte boundary and the row is a multiple of 4 floats.  Written as uint16 / float32 views of ONE byte buffer; the rounding is
tests/halo_bf16_ref.py's (nearest, ties to even), the routing tests/gatmh_bwd_merged_ref.py's.  numpy only: the GPU tests compare the
library's bytes with pack() and what it leaves in bg_do / bg_st with unpack(); tests/test_gatmh_halo_bf16_reference.py checks this
file against packing the rounded do and st separately."""
import numpy as np

import halo_bf16_ref as hb
from gatmh_bwd_merged_ref import pad_ld, route  # noqa: F401  (route: rows of wire_row()[0] floats travel like any others)


def wire_w(cols, exact):
    """the bf16 elements of do on the wire: its ld, or with halo_exact_rows its cols rounded up to a multiple of 8"""
    return (cols + 7) // 8 * 8 if exact else pad_ld(cols)


def wire_row(cols, K, exact):
    """(R, do_floats, 4K, w): 4-byte units of a merged row, of which the do part (w / 2), of which st; the bf16 elements of do"""
    w = wire_w(cols, exact)
    assert w % 8 == 0
    return w // 2 + 4 * K, w // 2, 4 * K, w


def pack(do, st, K, w, send_lists):
    """do: [N, cols] (zeros stand behind the columns up to w), st: [N, >= 4K]; send_lists: per peer, local vertex ids (a row may be
    listed for several peers).  Returns one float32 array of sum(len(list)) x (w / 2 + 4K): one byte buffer whose rows hold w uint16
    (the rounded do) and then 4K float32 (st, bit for bit)"""
    ids = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in send_lists]) if len(send_lists) else np.zeros(0, np.int64)
    do, st = np.ascontiguousarray(do, np.float32), np.ascontiguousarray(st, np.float32)
    assert w % 8 == 0 and st.shape[1] >= 4 * K
    R = w // 2 + 4 * K
    buf = np.zeros(ids.size * R * 4, np.uint8)
    rows = buf.reshape(ids.size, R * 4)
    n = min(w, do.shape[1])
    u16 = np.zeros((ids.size, w), np.uint16)
    u16[:, :n] = hb.round_bits(do[ids, :n])
    rows[:, :2 * w] = u16.view(np.uint8)
    rows[:, 2 * w:] = np.ascontiguousarray(st[ids, :4 * K]).view(np.uint8)
    return buf.view(np.float32)


def unpack(buf, K, w, recv_lists, G, ld, ld_st, bg_do=None, bg_st=None):
    """the received rows (peer order, then the peer's order) into ghost slots recv_lists[peer][k]: WHOLE rows of both tensors -- do
    widened into [0, w), st into [0, 4K), zeros into [w, ld) and [4K, ld_st), whatever they held.  Returns (bg_do [G, ld], bg_st
    [G, ld_st]); rows no list names keep what the given arrays hold (NaN where none is given)"""
    slots = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in recv_lists]) if len(recv_lists) else np.zeros(0, np.int64)
    R = w // 2 + 4 * K
    rows = np.ascontiguousarray(np.asarray(buf, np.float32).reshape(-1)[:slots.size * R]).view(np.uint8).reshape(slots.size, R * 4)
    bg_do = np.full((G, ld), np.nan, np.float32) if bg_do is None else np.array(bg_do, np.float32)
    bg_st = np.full((G, ld_st), np.nan, np.float32) if bg_st is None else np.array(bg_st, np.float32)
    bg_do[slots] = 0
    bg_st[slots] = 0
    bg_do[slots, :w] = hb.widen(np.ascontiguousarray(rows[:, :2 * w]).view(np.uint16))
    bg_st[slots, :4 * K] = np.ascontiguousarray(rows[:, 2 * w:]).view(np.float32)
    return bg_do, bg_st
