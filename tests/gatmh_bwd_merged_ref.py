"""Test-side restatement of the merged wire rows of dory_gatmh_bwd_merged_exchange (include/dorylus_hip.h): a sent local vertex v of
a multi-head GAT layer travels as ONE fp32 row [do[v, 0:w) | st[v, 0:4K)] of R = w + 4K floats, rows in the order of the backward
plan's send lists.  numpy only; the GPU tests compare the library's bytes with pack() and what it leaves in bg_do / bg_st with
unpack(), and tests/test_gatmh_bwd_merged_reference.py checks this file against routing the two tensors separately."""
import numpy as np


def pad_ld(cols):
    """the padded row width of a device tensor (csrc/ctx.hpp: pad_ld)"""
    return cols if cols <= 1 else (cols + 31) // 32 * 32


def wire_w(cols, exact):
    """the floats of do on the wire: its ld, or with halo_exact_rows its cols rounded up to a multiple of 4 (the columns past cols
    are the tensor's zero padding)"""
    return (cols + 3) // 4 * 4 if exact else pad_ld(cols)


def wire_row(cols, K, exact):
    """(R, w, 4K): floats of a merged row, of which do, of which st"""
    w = wire_w(cols, exact)
    return w + 4 * K, w, 4 * K


def _padded(t, width):
    t = np.ascontiguousarray(t, np.float32)
    out = np.zeros((t.shape[0], max(width, t.shape[1])), np.float32)
    out[:, :t.shape[1]] = t
    return out


def pack(do, st, K, w, send_lists):
    """do: [N, cols] (the tensor's columns; zeros stand behind them up to w), st: [N, >= 4K]; send_lists: per peer, local vertex ids.
    Returns one float32 array of sum(len(list)) x (w + 4K): the rows of all peers concatenated in peer order"""
    ids = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in send_lists]) if len(send_lists) else np.zeros(0, np.int64)
    d, s = _padded(do, w), np.ascontiguousarray(st, np.float32)
    assert s.shape[1] >= 4 * K and (w % 4) == 0
    out = np.zeros((ids.size, w + 4 * K), np.float32)
    out[:, :w] = d[ids, :w]
    out[:, w:] = s[ids, :4 * K]
    return out.reshape(-1)


def unpack(buf, K, w, recv_lists, G, ld, ld_st, bg_do=None, bg_st=None):
    """the received rows (peer order, then the peer's order) into ghost slots recv_lists[peer][k]: WHOLE rows of both tensors --
    [0, w) and [0, 4K) from the buffer, zeros into [w, ld) and [4K, ld_st), whatever they held.  Returns (bg_do [G, ld], bg_st
    [G, ld_st]); rows no list names keep what the given arrays hold (NaN where none is given)"""
    slots = np.concatenate([np.asarray(l, np.int64).reshape(-1) for l in recv_lists]) if len(recv_lists) else np.zeros(0, np.int64)
    R = w + 4 * K
    rows = np.asarray(buf, np.float32).reshape(-1)[:slots.size * R].reshape(slots.size, R)
    bg_do = np.full((G, ld), np.nan, np.float32) if bg_do is None else np.array(bg_do, np.float32)
    bg_st = np.full((G, ld_st), np.nan, np.float32) if bg_st is None else np.array(bg_st, np.float32)
    bg_do[slots] = 0
    bg_st[slots] = 0
    bg_do[slots, :w] = rows[:, :w]
    bg_st[slots, :4 * K] = rows[:, w:]
    return bg_do, bg_st


def route(send_bufs, row_floats, send_lists, recv_lists):
    """what an all-to-all-v does with P ranks' packed buffers: send_lists[r][p] are rank r's rows for peer p, recv_lists[p][r] the
    slots of rank p they land in (only their number is used).  Returns the P receive buffers (rows of row_floats floats)"""
    P = len(send_bufs)
    out = []
    for p in range(P):
        parts = []
        for r in range(P):
            n = len(send_lists[r][p])
            assert n == len(recv_lists[p][r]), (r, p, n, len(recv_lists[p][r]))
            off = sum(len(send_lists[r][q]) for q in range(p))
            parts.append(np.asarray(send_bufs[r], np.float32).reshape(-1)[off * row_floats:(off + n) * row_floats])
        out.append(np.concatenate(parts) if parts else np.zeros(0, np.float32))
    return out
