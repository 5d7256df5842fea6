"""The reference's scatter messages in numpy, written from its source: the sender loop (Engine::scatterGCN, engine/ops/gcn_ops.cpp:
204-260, scatterGAT, gat_ops.cpp:277-333, which call Engine::verticesPushOut, engine/utils.cpp:623-650, once per peer and batch)
and the receiver loop (ghostReceiverGCN, gcn_ops.cpp:284-318, ghostReceiverGAT, gat_ops.cpp:357-391).  No GPU, no library: what
tests/test_scatter_msg_format.py and tests/test_gpu_scatter_msgs.py compare dory_wire_*scatter* and dory_scatter_msgs_* with."""
import struct

import numpy as np

MAX_MSG_SIZE = 1 * 1024 * 1024        # engine/engine.hpp:24
NODE_ID_DIGITS = 8                    # engine.hpp:25
DATA_HEADER_SIZE = NODE_ID_DIGITS + 4 * 5   # engine.hpp:27


def batch_size(feat_dim, max_msg_bytes=0):
    """BATCH_SIZE (gcn_ops.cpp:225-228): std::max((MAX_MSG_SIZE - DATA_HEADER_SIZE) / (sizeof(unsigned) + sizeof(FeatType) * featDim), 1ul)"""
    max_msg = max_msg_bytes or MAX_MSG_SIZE
    return max(max(max_msg - DATA_HEADER_SIZE, 0) // (4 + 4 * feat_dim), 1)


def msg_bytes(rows, feat_dim):
    """zmq::message_t msg(DATA_HEADER_SIZE + (sizeof(unsigned) + sizeof(FeatType) * featDim) * totCnt)  (utils.cpp:626-628)"""
    return DATA_HEADER_SIZE + (4 + 4 * feat_dim) * rows


def header(receiver, sender, count, feat_dim, layer, direction):
    """sprintf(msgPtr, "%8X", receiver); populateHeader(msgPtr + 8, nodeId, totCnt, featDim, featLayer, c.dir)  (utils.cpp:630-640);
    the sender field overwrites the NUL sprintf leaves behind the eight characters"""
    return ("%8X" % receiver).encode("ascii") + struct.pack("<5I", sender, count, feat_dim, layer, direction)


def message(receiver, sender, lvids, local_to_global, tensor, feat_dim, layer, direction):
    """verticesPushOut for one batch: header, then per lvid its global id and featDim floats of the tensor's row (utils.cpp:642-648)"""
    lvids = np.asarray(lvids, np.int64)
    rec = np.empty((len(lvids), 1 + feat_dim), np.uint32)
    rec[:, 0] = np.asarray(local_to_global, np.uint32)[lvids]
    rec[:, 1:] = np.ascontiguousarray(tensor, np.float32)[lvids, :feat_dim].view(np.uint32)
    return header(receiver, sender, len(lvids), feat_dim, layer, direction) + rec.tobytes()


def send_messages(sender, send_lists, local_to_global, tensor, feat_dim, layer, direction, max_msg_bytes=0):
    """the loop over the peers and their batches (gcn_ops.cpp:237-257): [(receiver, message bytes)] in the order it sends them;
    send_lists[q]: the local ids whose rows peer q needs, in send-list order (batchedIds[q])"""
    out = []
    bs = batch_size(feat_dim, max_msg_bytes)
    for q, lst in enumerate(send_lists):
        if q == sender:
            continue
        for ib in range(0, len(lst), bs):
            out.append((q, message(q, sender, lst[ib:ib + bs], local_to_global, tensor, feat_dim, layer, direction)))
    return out


def parse(msg):
    """(receiver, sender, count, featDim, layer, dir, records as a (count, 1 + featDim) uint32 array) of one whole message"""
    assert len(msg) >= DATA_HEADER_SIZE
    receiver = int(bytes(msg[:8]).decode("ascii"), 16)
    sender, count, feat_dim, layer, direction = struct.unpack_from("<5I", msg, 8)
    assert len(msg) == msg_bytes(count, feat_dim)
    rec = np.frombuffer(msg, np.uint32, count * (1 + feat_dim), DATA_HEADER_SIZE).reshape(count, 1 + feat_dim)
    return receiver, sender, count, feat_dim, layer, direction, rec


def receive(ghost, ghost_gvids, msg):
    """the receiver loop for one message (gcn_ops.cpp:310-318): every record's floats to the ghost row of its global id
    (globalToGhostVtcs[gvid] - localVtxCnt = the id's position in the ghost list); returns the count (ghostVtcsRecvd += topic)"""
    _, _, count, feat_dim, _, _, rec = parse(msg)
    slot = {int(g): k for k, g in enumerate(ghost_gvids)}
    for r in rec:
        ghost[slot[int(r[0])], :feat_dim] = r[1:].view(np.float32)
    return count


def recut(msgs, batch):
    """the records of `msgs` (whole messages for one receiver with one header otherwise) in messages of `batch` records"""
    out = []
    for m in msgs:
        receiver, sender, count, feat_dim, layer, direction, rec = parse(m)
        for i in range(0, count, batch):
            part = rec[i:i + batch]
            out.append(header(receiver, sender, len(part), feat_dim, layer, direction) + part.tobytes())
    return out


def shuffled(msg, rng):
    """the same message with its records in another order"""
    receiver, sender, count, feat_dim, layer, direction, rec = parse(msg)
    return bytes(msg[:DATA_HEADER_SIZE]) + rec[rng.permutation(count)].tobytes()
