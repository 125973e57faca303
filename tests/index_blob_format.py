"""The saved-index format of include/mqvs.h (index persistence), restated in
numpy for the persistence tests: header pack / parse, the content's three
parts, and the grouping a load must produce from an assignment."""
import struct

import numpy as np

MAGIC = b"MQVSIDX\0"
HEADER = struct.Struct("<8sIIIIQQIIQ8s")  # 64 bytes
assert HEADER.size == 64
KIND_FLOAT, KIND_BINARY = 0, 1
IVF_PAD = 16  # float lists are padded to this many positions; binary lists are not


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


def pack_header(kind, metric, dim, n, nlist, alpha=3.0, np95=0, fingerprint=0, version=1, magic=MAGIC):
    return HEADER.pack(magic, version, kind, metric, dim, n, nlist, f32_bits(alpha), np95, fingerprint, b"\0" * 8)


def parse_header(content):
    magic, version, kind, metric, dim, n, nlist, alpha_bits, np95, fp, reserved = HEADER.unpack(content[:64])
    return dict(magic=magic, version=version, kind=kind, metric=metric, dim=dim, n=n, nlist=nlist,
                alpha=float(np.uint32(alpha_bits).view(np.float32)), np95=np95, fingerprint=fp, reserved=reserved)


def split_content(content):
    """-> (header dict, centroid bytes, assignment int32[n]); asserts the size the header implies."""
    h = parse_header(content)
    row = h["dim"] // 8 if h["kind"] == KIND_BINARY else 4 * h["dim"]
    cb = h["nlist"] * row
    assert len(content) == 64 + cb + 4 * h["n"], (len(content), h)
    return h, content[64:64 + cb], np.frombuffer(content[64 + cb:], np.int32)


def with_assignment(content, assign):
    """The content with its assignment section replaced."""
    h, cent, old = split_content(content)
    a = np.ascontiguousarray(assign, np.int32)
    assert a.shape == old.shape
    return content[:64] + cent + a.tobytes()


def np_lists(assign, nlist, pad):
    """(list_off int64[nlist + 1], rows int32[npos]) of an assignment: a stable
    sort of the rows by list id, every list's length rounded up to `pad`,
    unused positions -1."""
    assign = np.asarray(assign, np.int64)
    order = np.argsort(assign, kind="stable")
    order = order[assign[order] >= 0]
    cnt = np.bincount(assign[assign >= 0], minlength=nlist)
    off = np.concatenate([[0], np.cumsum((cnt + pad - 1) // pad * pad)]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)])
    rows = np.full(off[-1], -1, np.int32)
    for l in range(nlist):
        rows[off[l]:off[l] + cnt[l]] = order[start[l]:start[l + 1]]
    return off, rows
