"""The host-side format functions of the reference's scatter messages (include/dorylus_wire.h: dory_wire_scatter_batch,
dory_wire_scatter_msg_bytes, dory_wire_pack_scatter_header, dory_wire_parse_scatter_header) against the numpy restatement of the
reference's sender (tests/scatter_msg_ref.py) and, for bytes 8..28, against the reference's own populateHeader bytes
(fields_header of tests/golden/wire_headers.json).  CPU only."""
import ctypes as C
import json
import os
import struct

import pytest

import scatter_msg_ref as sm

RECEIVERS = (0, 10, 255, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def lib():
    import dorylus_amd
    assert os.path.exists(dorylus_amd.LIB_PATH), "the library is not built"
    lib = C.CDLL(dorylus_amd.LIB_PATH)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    lib.dory_wire_scatter_batch.argtypes = [u32, u64]
    lib.dory_wire_scatter_batch.restype = u32
    lib.dory_wire_scatter_msg_bytes.argtypes = [u32, u32]
    lib.dory_wire_scatter_msg_bytes.restype = u64
    lib.dory_wire_pack_scatter_header.argtypes = [vp, u32, u32, u32, u32, u32, u32]
    lib.dory_wire_pack_scatter_header.restype = None
    lib.dory_wire_parse_scatter_header.argtypes = [C.c_char_p, u64] + [C.POINTER(u32)] * 6
    lib.dory_wire_parse_scatter_header.restype = C.c_int
    return lib


def _pack(lib, *fields):
    buf = C.create_string_buffer(28)
    lib.dory_wire_pack_scatter_header(buf, *fields)
    return buf.raw


def _parse(lib, msg, nbytes=None):
    out = [C.c_uint32() for _ in range(6)]
    rc = lib.dory_wire_parse_scatter_header(bytes(msg), len(msg) if nbytes is None else nbytes, *[C.byref(x) for x in out])
    return rc, tuple(x.value for x in out)


def test_header_bytes_are_the_senders(lib):
    for receiver in RECEIVERS:
        for (sender, count, feat, layer, direction) in ((0, 1, 1, 0, 0), (3, 434, 602, 1, 0), (7, 2032, 128, 1, 1), (0xFFFFFFFE, 0xFFFFFFFF, 41, 2, 1)):
            got = _pack(lib, receiver, sender, count, feat, layer, direction)
            assert got == sm.header(receiver, sender, count, feat, layer, direction), (receiver, sender, count, feat, layer, direction)
            assert len(got) == sm.DATA_HEADER_SIZE == 28 and b"\0" not in got[:8]
    assert _pack(lib, 0, 0, 0, 0, 0, 0)[:8] == b"       0"
    assert _pack(lib, 10, 0, 0, 0, 0, 0)[:8] == b"       A"
    assert _pack(lib, 255, 0, 0, 0, 0, 0)[:8] == b"      FF"
    assert _pack(lib, 0xFFFFFFFF, 0, 0, 0, 0, 0)[:8] == b"FFFFFFFF"


def test_bytes_8_to_28_are_the_references_fields_header(lib, golden_dir):
    gold = json.load(open(os.path.join(golden_dir, "wire_headers.json")))
    assert gold["cases"]
    for c in gold["cases"]:
        for receiver in RECEIVERS:
            got = _pack(lib, receiver, c["op"], c["f1"], c["f2"], c["f3"], c["f4"])
            assert got[8:28].hex() == c["fields_header"], c
            assert got[:8] == ("%8X" % receiver).encode()


def test_batch_rule(lib):
    # the reference's message size: the four counts of the issue, and a feature width of 1
    for feat, want in ((128, 2032), (602, 434), (41, 6241), (48, 5349), (1, (1048576 - 28) // 8)):
        assert lib.dory_wire_scatter_batch(feat, 0) == want == sm.batch_size(feat), feat
        assert lib.dory_wire_scatter_batch(feat, 1048576) == want
        assert lib.dory_wire_scatter_msg_bytes(want, feat) <= 1048576 < lib.dory_wire_scatter_msg_bytes(want + 1, feat)
    for feat in (1, 41, 48, 128, 602):
        rec = 4 + 4 * feat
        for max_msg in (1, 27, 28, 28 + rec - 1, 28 + rec, 28 + 3 * rec, 28 + 3 * rec + rec - 1, 28 + 4 * rec, 65536, 0xFFFFFFFF):
            assert lib.dory_wire_scatter_batch(feat, max_msg) == sm.batch_size(feat, max_msg), (feat, max_msg)
        assert lib.dory_wire_scatter_batch(feat, rec - 1) == 1 and lib.dory_wire_scatter_batch(feat, 28 + rec - 1) == 1   # smaller than one record
        assert lib.dory_wire_scatter_batch(feat, 28 + 3 * rec) == 3
        for rows in (0, 1, 7, 434):
            assert lib.dory_wire_scatter_msg_bytes(rows, feat) == sm.msg_bytes(rows, feat) == 28 + rows * rec


def test_parser_takes_the_senders_messages_and_refuses_the_rest(lib):
    import numpy as np
    feat, rows = 5, 3
    x = np.arange(40, dtype=np.float32).reshape(8, 5)
    msg = sm.message(10, 2, [1, 4, 4], np.arange(100, 108), x, feat, 1, 0)
    assert len(msg) == 28 + rows * 24
    assert _parse(lib, msg) == (0, (10, 2, rows, feat, 1, 0))
    for receiver in RECEIVERS:
        m = sm.header(receiver, 1, 0, 7, 3, 1)
        assert _parse(lib, m) == (0, (receiver, 1, 0, 7, 3, 1))
    # null outputs are allowed
    assert lib.dory_wire_parse_scatter_header(msg, len(msg), None, None, None, None, None, None) == 0
    # a short buffer
    for n in (0, 1, 27):
        assert _parse(lib, msg[:n])[0] == -1, n
    assert lib.dory_wire_parse_scatter_header(None, 100, None, None, None, None, None, None) == -1
    # bytes that are not 28 + count x (4 + 4 featDim): truncated, one byte off, one record more or less
    for n in (28, len(msg) - 24, len(msg) - 1, len(msg) - 4):
        assert _parse(lib, msg[:n])[0] == -1, n
    assert _parse(lib, msg + b"\0")[0] == -1 and _parse(lib, msg + msg[-24:])[0] == -1
    assert _parse(lib, msg, len(msg) + 24)[0] == -1
    # a receiver field that is not eight characters of %8X
    for bad in (b"0000000A", b"       a", b"A       ", b"        ", b"\0\0\0\0\0\0\0A", b"      0A", b"   1 2 3", b"      -1", b"0x00000A", b"       G"):
        assert len(bad) == 8
        assert _parse(lib, bad + msg[8:])[0] == -1, bad
    for good, val in ((b"       A", 10), (b"      10", 16), (b"FFFFFFFF", 0xFFFFFFFF), (b"       0", 0), (b" 1234ABC", 0x1234ABC)):
        assert _parse(lib, good + msg[8:]) == (0, (val, 2, rows, feat, 1, 0)), good
    assert struct.unpack_from("<5I", msg, 8) == (2, rows, feat, 1, 0)
