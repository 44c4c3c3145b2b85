"""The tree of a leaf set (include/rgbdfe.h, "the tree of a leaf set"): two formulations that share no code, and an
independent reader of .ot files.

  LiteralTree   a pointer tree of dicts: every leaf descends from the root as OcTreeBaseImpl::updateNode does
                (computeChildIdx per depth, nodes created on the way), then updateInnerOccupancyRecurs
                (updateOccupancyChildren = getMaxChildLogOdds, updateColorChildren = getAverageChildColor), then the
                recursive writeData of an .ot file.
  flat_tree     numpy over arrays: path codes, one sort, the shared prefix of neighbours, sixteen level passes with
                reduceat, records scattered to their pre-order positions.
  read_ot       a recursive reader that follows the child masks back down to the leaves.

Leaves are octomap_oracle.LEAF records; node records are NODE (float32 log-odds, rgb[3], child mask): 8 bytes."""
import numpy as np

from octomap_oracle import LEAF

NODE = np.dtype([("log_odds", "<f4"), ("rgb", "u1", (3,)), ("children", "u1")])
FLT_MAX = np.float32(3.4028234663852886e38)


def header(n_nodes, resolution):
    return ("# Octomap OcTree file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
            "id ColorOcTree\nsize %d\nres %g\ndata\n" % (n_nodes, resolution)).encode()


def ot_file(records, resolution):
    return header(len(records), resolution) + records.tobytes()


# ------------------------------------------------------------------------------------------------ the literal tree
class LiteralTree:
    def __init__(self, leaves=()):
        self.root = None
        for l in leaves:
            self.update_node(tuple(int(k) for k in l["key"]), np.float32(l["log_odds"]), tuple(int(c) for c in l["rgb"]))
        self.update_inner_occupancy()

    @staticmethod
    def new_node():
        return {"children": [None] * 8, "value": np.float32(0.0), "rgb": (255, 255, 255)}

    def update_node(self, key, value, rgb):
        if self.root is None:
            self.root = self.new_node()
        node = self.root
        for depth in range(1, 17):
            b = 16 - depth
            pos = ((key[0] >> b) & 1) | (((key[1] >> b) & 1) << 1) | (((key[2] >> b) & 1) << 2)  # computeChildIdx
            if node["children"][pos] is None:
                node["children"][pos] = self.new_node()
            node = node["children"][pos]
        node["value"], node["rgb"] = value, rgb

    def update_inner_occupancy(self):
        if self.root is not None:
            self._inner(self.root, 0)

    def _inner(self, node, depth):
        kids = [c for c in node["children"] if c is not None]
        if not kids:
            return
        if depth < 16:
            for c in kids:
                self._inner(c, depth + 1)
        mx = -FLT_MAX  # getMaxChildLogOdds
        for c in kids:
            if c["value"] > mx:
                mx = c["value"]
        node["value"] = np.float32(mx)
        mr = mg = mb = n = 0  # getAverageChildColor
        for c in kids:
            if c["rgb"] != (255, 255, 255):  # isColorSet
                mr += c["rgb"][0]
                mg += c["rgb"][1]
                mb += c["rgb"][2]
                n += 1
        node["rgb"] = (mr // n, mg // n, mb // n) if n > 0 else (255, 255, 255)

    def records(self):
        """writeData: node, child mask, then the children in ascending index."""
        out = []
        if self.root is not None:
            self._write(self.root, out)
        rec = np.zeros(len(out), NODE)
        for i, (v, c, m) in enumerate(out):
            rec["log_odds"][i], rec["rgb"][i], rec["children"][i] = v, c, m
        return rec

    def _write(self, node, out):
        mask = sum(1 << i for i in range(8) if node["children"][i] is not None)
        out.append((node["value"], node["rgb"], mask))
        for c in node["children"]:
            if c is not None:
                self._write(c, out)

    def at_depth(self, depth):
        """The nodes of one depth in tree order as LEAF records (key: the node's cells' common bits, the rest 0)."""
        out = []

        def walk(node, d, key):
            if d == depth:
                out.append((key, node["value"], node["rgb"]))
                return
            b = 15 - d
            for i, c in enumerate(node["children"]):
                if c is not None:
                    walk(c, d + 1, (key[0] | ((i & 1) << b), key[1] | (((i >> 1) & 1) << b), key[2] | (((i >> 2) & 1) << b)))

        if self.root is not None:
            walk(self.root, 0, (0, 0, 0))
        rec = np.zeros(len(out), LEAF)
        for i, (k, v, c) in enumerate(out):
            rec["key"][i], rec["log_odds"][i], rec["rgb"][i] = k, v, c
        return rec


# ------------------------------------------------------------------------------------------------ the flat form
def path_codes(keys):
    """[n, 3] uint16 keys -> uint64 codes: bit b of key[a] at bit 3 b + a."""
    k = np.asarray(keys, np.uint64).reshape(-1, 3)
    code = np.zeros(len(k), np.uint64)
    for b in range(16):
        for a in range(3):
            code |= ((k[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return code


def keys_of_codes(code, depth):
    k = np.zeros((len(code), 3), np.uint16)
    for b in range(16 - depth, 16):
        for a in range(3):
            k[:, a] |= (((code >> np.uint64(3 * b + a)) & np.uint64(1)) << np.uint64(b)).astype(np.uint16)
    return k


def flat_tree(leaves):
    """(records in pre-order, {depth: LEAF records of that depth in tree order})."""
    n = len(leaves)
    if n == 0:
        return np.zeros(0, NODE), {d: np.zeros(0, LEAF) for d in range(17)}
    code = path_codes(leaves["key"])
    order = np.argsort(code, kind="stable")
    code = code[order]
    value = leaves["log_odds"][order].astype(np.float32)
    rgb = leaves["rgb"][order].astype(np.int64)
    # top[j]: the shallowest depth whose node starts at leaf j
    top = np.zeros(n, np.int64)
    x = code[1:] ^ code[:-1]
    assert np.all(x != 0), "a repeated key"
    t1 = np.full(len(x), 17, np.int64)
    for d in range(16, 0, -1):  # the shallowest depth at which the child indices of the two leaves differ
        t1 = np.where((x >> np.uint64(3 * (16 - d))) != 0, d, t1)
    top[1:] = t1
    off = np.concatenate([[0], np.cumsum(17 - top)[:-1]])
    total = int(np.sum(17 - top))
    rec = np.zeros(total, NODE)
    levels = {}
    first = np.arange(n)
    mask = np.zeros(n, np.int64)
    for d in range(16, -1, -1):
        at = off[first] + (d - top[first])
        rec["log_odds"][at], rec["rgb"][at], rec["children"][at] = value, rgb, mask
        lv = np.zeros(len(first), LEAF)
        lv["key"], lv["log_odds"], lv["rgb"] = keys_of_codes(code[first], d), value, rgb
        levels[d] = lv
        if d == 0:
            break
        head = np.nonzero(top[first] <= d - 1)[0]  # the children that start a parent of depth d - 1
        child = ((code[first] >> np.uint64(3 * (16 - d))) & np.uint64(7)).astype(np.int64)
        mask = np.add.reduceat(np.int64(1) << child, head)
        value = np.maximum.reduceat(value, head)
        is_set = np.any(rgb != 255, axis=1)
        cnt = np.add.reduceat(is_set.astype(np.int64), head)
        sums = np.add.reduceat(rgb * is_set[:, None], head, axis=0)
        rgb = np.where(cnt[:, None] > 0, sums // np.maximum(cnt, 1)[:, None], 255)
        first = first[head]
    return rec, levels


# ------------------------------------------------------------------------------------------------ the reader
def read_ot(blob):
    """(id, size, res text, LEAF records in ascending packed key) of an .ot file; raises ValueError on a malformed one."""
    lines, at = [], 0
    while True:
        e = blob.index(b"\n", at)
        line = blob[at:e].decode()
        at = e + 1
        if line == "data":
            break
        lines.append(line)
    if not lines or not lines[0].startswith("# Octomap OcTree file"):
        raise ValueError("first line")
    fields = dict(l.split(" ", 1) for l in lines if not l.startswith("#"))
    size = int(fields["size"])
    data = blob[at:]
    found = []
    pos = [0]

    def node(depth, key):
        if pos[0] + 8 > len(data):
            raise ValueError("truncated")
        r = np.frombuffer(data, NODE, 1, pos[0])[0]
        pos[0] += 8
        m = int(r["children"])
        if depth == 16:
            if m:
                raise ValueError("children below depth 16")
            found.append((key, r["log_odds"], tuple(r["rgb"])))
            return 1
        if not m:
            raise ValueError("pruned")
        b, cnt = 15 - depth, 1
        for i in range(8):
            if (m >> i) & 1:
                cnt += node(depth + 1, (key[0] | ((i & 1) << b), key[1] | (((i >> 1) & 1) << b), key[2] | (((i >> 2) & 1) << b)))
        return cnt

    walked = node(0, (0, 0, 0)) if size > 0 else 0
    if walked != size or pos[0] != len(data):
        raise ValueError("size")
    found.sort(key=lambda it: it[0][0] | (it[0][1] << 16) | (it[0][2] << 32))
    out = np.zeros(len(found), LEAF)
    for i, (k, v, c) in enumerate(found):
        out["key"][i], out["log_odds"][i], out["rgb"][i] = k, v, c
    return fields["id"], size, fields["res"], out


# ------------------------------------------------------------------------------------------------ planted leaf sets
def leaf_records(items):
    """[((k0, k1, k2), log-odds, (r, g, b))] -> LEAF records in the given order."""
    out = np.zeros(len(items), LEAF)
    for i, (k, v, c) in enumerate(items):
        out["key"][i], out["log_odds"][i], out["rgb"][i] = k, v, c
    return out


def random_leaves(n, seed):
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < n:
        # half of the keys close together (deep shared prefixes), half anywhere
        if rng.random() < 0.5:
            keys.add(tuple(int(v) for v in 32768 + rng.integers(-6, 6, 3)))
        else:
            keys.add(tuple(int(v) for v in rng.integers(0, 65536, 3)))
    keys = list(keys)
    rng.shuffle(keys)
    out = []
    for k in keys:
        c = (255, 255, 255) if rng.random() < 0.2 else tuple(int(v) for v in rng.integers(0, 256, 3))
        out.append((k, np.float32(rng.uniform(-3.0, 3.0)), c))
    return leaf_records(out)


def planted_sets():
    """(name, LEAF records): the smallest inputs on which each rule of the contract can go wrong."""
    W = (255, 255, 255)
    B = 32768
    sets = []
    sets.append(("one leaf", leaf_records([((12345, 54321, 777), 0.85, (10, 20, 30))])))
    # eight siblings: channel sums not divisible by 6, two white
    sib = [((B + (i & 1), B + ((i >> 1) & 1), B + ((i >> 2) & 1)), 0.1 * i - 0.3, W if i in (2, 5) else (10 + 3 * i, 7 * i, 255 - i))
           for i in range(8)]
    sets.append(("eight siblings", leaf_records(sib)))
    # three coloured leaves in one depth-15 octant, one in its sibling: flat mean (1+2+2+200)/4 = 51, hierarchical
    # (floor(5/3) + 200) / 2 = 100
    sets.append(("hierarchical average", leaf_records([((B, B, B), 0.5, (1, 1, 1)), ((B + 1, B, B), 0.5, (2, 2, 2)),
                                                       ((B, B + 1, B), 0.5, (2, 2, 2)), ((B + 2, B, B), 0.5, (200, 100, 0))])))
    sets.append(("negative only", leaf_records([((100, 200, 300), -0.4, (1, 2, 3)), ((101, 200, 300), -2.0, (4, 5, 6)),
                                                ((100, 9000, 300), -1.5, W)])))
    # a subtree of white leaves beside a coloured one: the white parent must not count one level up
    sets.append(("white subtree", leaf_records([((B, B, B), 0.2, W), ((B + 1, B, B), 0.3, W), ((B + 2, B, B), 0.4, (90, 60, 31)),
                                                ((B + 2, B + 1, B), 0.4, (31, 61, 90))])))
    sets.append(("root only shared", leaf_records([((0, 0, 0), 1.0, (1, 2, 3)), ((65535, 65535, 65535), -1.0, (250, 251, 252)),
                                                   ((32767, 32767, 32767), 0.5, (9, 9, 9)), ((32768, 32768, 32768), 2.0, W)])))
    for n in (1, 255, 256, 257, 1025):
        sets.append(("random %d" % n, random_leaves(n, 100 + n)))
    return sets
