"""A writer and a reader of session files, written from the format's description in include/rgbdfe.h ("session files") with
struct and zlib.crc32 -- not from the C++ code.  tests/test_session_format_host.py makes the validator's inputs with the
writer; tests/test_gpu_session.py reads the library's files with the reader."""
import struct
import zlib

import numpy as np

MAGIC, VERSION, CLOUDS = b"RGBDFESS", 1, 1
ORDER = [b"CONF", b"DETE", b"NODE", b"CLOU", b"GRPH", b"SLAM", b"END "]
DESC_ROW = {0: 32, 1: 512, 2: 512}


def pad8(b):
    return b + bytes(-len(b) % 8)


def chunk(tag, payload):
    return tag + struct.pack("<IQ", zlib.crc32(payload), len(payload)) + pad8(payload)


def assemble(flags, chunks):
    """chunks: (tag, payload) in file order; the END chunk and the header's length are added."""
    body = b"".join(chunk(t, p) for t, p in chunks) + chunk(b"END ", b"")
    return MAGIC + struct.pack("<IIQQ", VERSION, flags, 32 + len(body), 0) + body


def conf_payload(max_keypoints, abi, kinds):
    return struct.pack("<iiII", max_keypoints, abi, sum(1 << k for k in set(kinds)), 0)


def dete_payload(detector_type=0, max_keypoints=600, grid=3, iters=5, min_depth=0, thresholds=None):
    t = np.full(grid * grid, 20.0) if thresholds is None else np.asarray(thresholds, np.float64)
    return struct.pack("<6i", detector_type, max_keypoints, grid, iters, min_depth, len(t)) + t.tobytes()


def node_payload(nodes):
    """nodes: {id: dict(kind, desc, xyz1, kp_xy or None, stats)}."""
    ids = sorted(nodes)
    n = len(ids)
    out = struct.pack("<II", n, 0)
    out += np.array(ids, "<i4").tobytes() + np.array([nodes[i]["kind"] for i in ids], "<i4").tobytes()
    out += np.array([len(nodes[i]["xyz1"]) for i in ids], "<i4").tobytes()
    out += np.array([int(nodes[i].get("kp_xy") is not None) for i in ids], "<i4").tobytes()
    for kind in (0, 1, 2):
        mine = [nodes[i] for i in ids if nodes[i]["kind"] == kind]
        if not mine:
            continue
        kp = [m["kp_xy"] if m.get("kp_xy") is not None else np.zeros((len(m["xyz1"]), 2), np.float32) for m in mine]
        for arrays in ([m["desc"] for m in mine], [m["xyz1"] for m in mine], kp, [m["stats"] for m in mine]):
            out = pad8(out + b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
    return out


def clou_payload(clouds):
    """clouds: {id: dict(points [rows, cols, 4] f32, cloud_skip, fx, fy, cx, cy)}."""
    out = struct.pack("<II", len(clouds), 0)
    for i in sorted(clouds):
        c = clouds[i]
        rows, cols = c["points"].shape[:2]
        out += struct.pack("<4i4f", i, rows, cols, c["cloud_skip"], c["fx"], c["fy"], c["cx"], c["cy"])
        out += np.ascontiguousarray(c["points"], "<f4").tobytes()
    return out


def write(max_keypoints, abi, nodes, dete=None, clouds=None, graph=None, slam=None):
    chunks = [(b"CONF", conf_payload(max_keypoints, abi, [m["kind"] for m in nodes.values()])), (b"DETE", dete or dete_payload()),
              (b"NODE", node_payload(nodes))]
    if clouds is not None:
        chunks.append((b"CLOU", clou_payload(clouds)))
    if graph is not None:
        chunks.append((b"GRPH", graph))
    if slam is not None:
        chunks.append((b"SLAM", slam))
    return assemble(CLOUDS if clouds is not None else 0, chunks)


def chunk_table(b):
    """[(tag, payload offset, payload length)] of a file, its header and every CRC checked."""
    assert b[:8] == MAGIC
    version, flags, length, zero = struct.unpack_from("<IIQQ", b, 8)
    assert version == VERSION and length == len(b) and zero == 0
    at, table = 32, []
    while True:
        tag = b[at:at + 4]
        crc, n = struct.unpack_from("<IQ", b, at + 4)
        assert zlib.crc32(b[at + 16:at + 16 + n]) == crc, tag
        table.append((tag, at + 16, n))
        at += 16 + n + (-n % 8)
        if tag == b"END ":
            break
    assert at == len(b) and [t for t, _, _ in table] == [t for t in ORDER if t in [x for x, _, _ in table]]
    return flags, table


def read(b):
    """A file as dict(flags, max_keypoints, abi, kinds, dete, nodes {id: ...}, clouds {id: ...}, graph, slam)."""
    flags, table = chunk_table(b)
    at = {t: (o, n) for t, o, n in table}
    out = dict(flags=flags, table=table, graph=None, slam=None, clouds=None)
    o, n = at[b"CONF"]
    assert n == 16
    out["max_keypoints"], out["abi"], out["kinds"], zero = struct.unpack_from("<iiII", b, o)
    o, n = at[b"DETE"]
    t, mk, grid, iters, md, cells = struct.unpack_from("<6i", b, o)
    assert n == 24 + 8 * cells
    out["dete"] = dict(type=t, max_keypoints=mk, grid=grid, iters=iters, min_depth=md, thresholds=np.frombuffer(b, "<f8", cells, o + 24))
    o, n = at[b"NODE"]
    end = o + n
    count, zero = struct.unpack_from("<II", b, o)
    cols = [np.frombuffer(b, "<i4", count, o + 8 + 4 * count * k) for k in range(4)]
    p = o + 8 + 16 * count
    nodes = {}
    for kind in (0, 1, 2):
        mine = [k for k in range(count) if cols[1][k] == kind]
        if not mine:
            continue
        total = int(sum(cols[2][k] for k in mine))
        arrays = []
        for width in (DESC_ROW[kind], 16, 8, 1):
            arrays.append(b[p:p + total * width])
            p += total * width
            p += -(p - o) % 8
        row = 0
        for k in mine:
            r = int(cols[2][k])
            cut = lambda a, w: a[row * w:(row + r) * w]
            nodes[int(cols[0][k])] = dict(kind=kind, rows=r, has_kp=int(cols[3][k]), desc=cut(arrays[0], DESC_ROW[kind]), xyz1=cut(arrays[1], 16),
                                          kp_xy=cut(arrays[2], 8), stats=cut(arrays[3], 1))
            row += r
    assert p == end and list(cols[0]) == sorted(cols[0])
    out["nodes"] = nodes
    if b"CLOU" in at:
        o, n = at[b"CLOU"]
        count, zero = struct.unpack_from("<II", b, o)
        p, clouds = o + 8, {}
        for _ in range(count):
            i, rows, cols_, skip, fx, fy, cx, cy = struct.unpack_from("<4i4f", b, p)
            p += 32
            clouds[i] = dict(rows=rows, cols=cols_, cloud_skip=skip, fx=fx, fy=fy, cx=cx, cy=cy, points=b[p:p + 16 * rows * cols_])
            p += 16 * rows * cols_
        assert p == o + n
        out["clouds"] = clouds
    for tag, key in ((b"GRPH", "graph"), (b"SLAM", "slam")):
        if tag in at:
            out[key] = b[at[tag][0]:at[tag][0] + at[tag][1]]
    return out
