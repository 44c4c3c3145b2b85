"""-m gpu: the tree of an occupancy map's leaves (include/rgbdfe.h, "the tree of a leaf set"; csrc/octomap_tree.hip and
the tree entry points of csrc/api_octomap.hip) through the C ABI against tests/octomap_tree_oracle.py.  Every comparison
is on bytes: node records, whole .ot files, the records of one depth.  The families are those of octomap_oracle.cases();
their reference is the flat formulation, which tests/test_oracle_octomap_tree.py holds equal to the literal pointer tree
on the same maps; the planted leaf sets are compared with the literal tree itself."""
import numpy as np
import pytest

import octomap_oracle as oo
import octomap_tree_oracle as to

pytestmark = pytest.mark.gpu

CASES = oo.cases()
PLANTED = to.planted_sets()
DEPTHS = (0, 1, 8, 15, 16)
_REF = {}


def want(case):
    """(leaves, records, levels) of a family, computed once."""
    if case[0] not in _REF:
        leaves = oo.run(case).leaves()
        _REF[case[0]] = (leaves,) + to.flat_tree(leaves)
    return _REF[case[0]]


def case_named(name):
    return [c for c in CASES if c[0] == name][0]


@pytest.fixture(scope="module")
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=16, max_keypoints=64, max_pairs_per_batch=16)
    yield f
    f.close()


def home_slot(key, cap):
    """Host twin of home_slot (csrc/octomap.hip): the first slot a key is tried at in a table of `cap` slots."""
    k = np.asarray(key, np.uint64)
    h = k[:, 0] | (k[:, 1] << np.uint64(16)) | (k[:, 2] << np.uint64(32))
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    return (((h >> np.uint64(32)) * np.uint64(cap)) >> np.uint64(32)).astype(np.int64)


def occupied_slots(home, cap):
    """The slots that hold a leaf in a table of `cap` slots: with linear probing the set does not depend on the order in
    which the leaves went in."""
    taken = set()
    for h in home:
        s = int(h)
        while s in taken:
            s = s + 1 if s + 1 < cap else 0
        taken.add(s)
    return np.array(sorted(taken))


# two keys found by search: the first has slot 2^20, the one slot of tile 1024, in a table of 2^20 + 1 slots; the second a
# slot behind 2^21, in the third trip, in a table of 2^21 + 1025
LATE_SLOT_LEAVES = to.leaf_records([((48479, 63624, 53141), np.float32(0.75), (200, 100, 50)),
                                    ((50595, 28226, 26079), np.float32(-1.25), (3, 2, 1))])


def rowmajor(T):
    return np.asarray(T, np.float32).reshape(4, 4).T


def insert(m, ins):
    for pts, T, mr in ins:
        m.insert_cloud(pts, rowmajor(T), mr)


def same(got, ref, what="records"):
    assert got.dtype == ref.dtype and len(got) == len(ref), (what, len(got), len(ref))
    if got.tobytes() != ref.tobytes():
        bad = np.nonzero(got != ref)[0]
        raise AssertionError("%s: %d of %d differ; the first at %d: got %s, want %s" % (what, len(bad), len(ref), bad[0], got[bad[0]],
                                                                                        ref[bad[0]]))


def check_depths(m, level_of):
    """nodes_at_depth against the level records: every node, the non-negative ones, and a threshold that occurs."""
    for d in DEPTHS:
        lv = level_of(d)
        same(m.nodes_at_depth(d), lv, "depth %d, -inf" % d)
        same(m.nodes_at_depth(d, 0.0), lv[lv["log_odds"] >= np.float32(0.0)], "depth %d, 0.0" % d)
        if len(lv):
            thr = np.sort(lv["log_odds"])[len(lv) // 2]  # a value that occurs: >= keeps it
            keep = lv[lv["log_odds"] >= thr]
            assert np.any(keep["log_odds"] == thr)
            same(m.nodes_at_depth(d, float(thr)), keep, "depth %d, %r" % (d, thr))


def check_file(m, tmp_path, records, resolution):
    path = tmp_path / "map.ot"
    m.write(str(path))
    assert path.read_bytes() == to.ot_file(records, resolution)
    return path


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_tree_file_and_depths_of_every_family(fe, case, tmp_path):
    leaves, rec, levels = want(case)
    with fe.octomap(2 * len(leaves) + 64, **case[1]) as m:
        insert(m, case[2])
        same(m.tree(), rec)
        check_file(m, tmp_path, rec, m.params.resolution)
        check_depths(m, lambda d: levels[d])
        same(m.leaves(), leaves, "the leaves after the tree calls")


def path_order(leaves):
    return leaves[np.argsort(to.path_codes(leaves["key"]), kind="stable")]


def test_depth_16_is_the_leaves_in_path_order(fe):
    case = case_named("n 3072 res 0.1 range 2.8")
    leaves = want(case)[0]
    with fe.octomap(2 * len(leaves), **case[1]) as m:
        insert(m, case[2])
        got = m.nodes_at_depth(16)
        same(got, path_order(m.leaves()), "depth 16")
        assert sorted(got.tobytes()[i:i + 16] for i in range(0, 16 * len(got), 16)) == \
            sorted(leaves.tobytes()[i:i + 16] for i in range(0, 16 * len(leaves), 16))


@pytest.mark.parametrize("name,leaves", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_leaf_sets(fe, name, leaves, tmp_path):
    lit = to.LiteralTree(leaves)
    rec = lit.records()
    with fe.octomap(len(leaves) + 3) as m:
        m.set_leaves(leaves)
        assert len(m) == len(leaves)
        same(m.leaves(), oo.records([(oo.pack(*l["key"]), l["log_odds"], tuple(l["rgb"])) for l in leaves]), "leaves")
        same(m.tree(), rec)
        check_file(m, tmp_path, rec, 0.05)
        check_depths(m, lit.at_depth)
    if name == "one leaf":
        assert len(rec) == 17


def test_tree_device_writes_the_same_records(fe):
    import torch
    case = case_named("n 1025 res 0.05 range -1")
    leaves, rec, _ = want(case)
    with fe.octomap(2 * len(leaves), **case[1]) as m:
        insert(m, case[2])
        out = torch.full((len(rec) + 5, 8), 0xAB, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()  # the fill runs on torch's stream, the tree on the context's
        assert m.tree_device(out) == len(rec)
        host = out.cpu().numpy()
        assert host[:len(rec)].tobytes() == rec.tobytes() and np.all(host[len(rec):] == 0xAB)
        small = torch.full((len(rec) - 1, 8), 0xAB, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        with pytest.raises(Exception, match="capacity"):
            m.tree_device(small)
        assert np.all(small.cpu().numpy() == 0xAB)


def test_short_buffer_empty_map_and_launch_count(fe, tmp_path):
    from rgbdslam_v2_amd import _lib
    case = case_named("n 257 res 0.1 range -1")
    leaves, rec, levels = want(case)
    with fe.octomap(2 * len(leaves), **case[1]) as m:
        # empty: no node, not even a root; a header-only file
        assert len(m.tree()) == 0 and all(len(m.nodes_at_depth(d)) == 0 for d in DEPTHS)
        check_file(m, tmp_path, np.zeros(0, to.NODE), 0.1)
        insert(m, case[2])
        short = np.zeros(len(rec) - 1, _lib.OCTOMAP_NODE_DTYPE)
        short["children"] = 0x5a
        st, need = m.tree_status(short)
        assert (st, need) == (-5, len(rec)) and np.all(short["children"] == 0x5a) and np.all(short["log_odds"] == 0)
        same(m.tree(), rec)
        small = m.last_tree_launches
    big_case = case_named("n 3072 res 0.05 range -1")
    with fe.octomap(2 * len(want(big_case)[0]), **big_case[1]) as m:
        insert(m, big_case[2])
        m.tree()
        assert m.last_tree_launches == small  # the launches of a call do not depend on the map's size


def test_the_table_does_not_show(fe):
    case = case_named("n 1025 res 0.1 range 2.8")
    leaves, rec, _ = want(case)
    for cap in (len(leaves), len(leaves) + 1, 3 * len(leaves) + 17):
        with fe.octomap(cap, **case[1]) as m:
            m.set_leaves(leaves)
            same(m.tree(), rec, "capacity %d" % cap)
    # tables of more than 1024 slot tiles: tree_scan_kernel's later trips over the gather stage's counts
    leaves = np.concatenate([dict(PLANTED)["random 1025"], LATE_SLOT_LEAVES])
    lit = to.LiteralTree(leaves)
    rec = lit.records()
    for cap, n_trips in ((2**20, 1), (2**20 + 1, 2), (2**21 + 1025, 3)):
        taken = occupied_slots(home_slot(leaves["key"], cap), cap)
        assert -(-(-(-cap // 1024)) // 1024) == n_trips
        for trip in range(1, n_trips):  # leaves in the slots of every later trip: their rows need the carried base
            assert np.any((taken >= trip * 2**20) & (taken < (trip + 1) * 2**20))
        with fe.octomap(cap) as m:
            m.set_leaves(leaves)
            same(m.tree(), rec, "capacity %d" % cap)
            same(m.nodes_at_depth(16), lit.at_depth(16), "depth 16, capacity %d" % cap)


def test_a_tree_call_between_inserts_changes_nothing(fe):
    case = case_named("other probabilities")
    leaves, rec, _ = want(case)
    ins = case[2]
    with fe.octomap(2 * len(leaves), **case[1]) as m:
        insert(m, ins[:4])
        first = m.tree()
        m.nodes_at_depth(8)
        insert(m, ins[4:])
        same(m.leaves(), leaves, "leaves")
        same(m.tree(), rec, "the second tree")  # the new leaves: nothing stale
        assert first.tobytes() != rec.tobytes()


def test_write_read_round_trip_and_resume(fe, tmp_path):
    case = case_named("other probabilities")
    leaves, rec, _ = want(case)
    ins = case[2]
    with fe.octomap(4 * len(leaves), **case[1]) as a, fe.octomap(2 * len(leaves), **case[1]) as b:
        insert(a, ins[:4])
        path = tmp_path / "half.ot"
        a.write(str(path))
        b.read(str(path))
        same(b.leaves(), a.leaves(), "leaves read back")
        insert(b, ins[4:])
        same(b.leaves(), leaves, "the resumed run")
        same(b.tree(), rec, "the resumed run's tree")


def test_read_refusals(fe, tmp_path):
    leaves = [l for n, l in PLANTED if n == "eight siblings"][0]
    rec = to.LiteralTree(leaves).records()
    good = to.ot_file(rec, 0.05)
    pruned = rec[:16].copy()
    pruned["children"][15] = 0
    deep = rec.copy()
    deep["children"][16] = 1
    files = {
        "id": good.replace(b"id ColorOcTree", b"id OcTree"),
        "res": good.replace(b"res 0.05", b"res 0.1"),
        "truncated": good[:-8],
        "size": good.replace(b"size 24", b"size 25"),
        "pruned": to.ot_file(pruned, 0.05),
        "depth 16": to.ot_file(deep, 0.05),
    }
    with fe.octomap(64) as m:
        m.set_leaves(leaves[:3])
        before = m.leaves()
        for word, blob in files.items():
            path = tmp_path / "bad.ot"
            path.write_bytes(blob)
            with pytest.raises(Exception, match="invalid argument.*" + word):
                m.read(str(path))
            same(m.leaves(), before, "the map after a refused file")
        with pytest.raises(Exception, match="invalid argument"):
            m.read(str(tmp_path / "missing.ot"))
        path = tmp_path / "good.ot"
        path.write_bytes(good)
        m.read(str(path))
        same(m.tree(), rec)
        with pytest.raises(Exception, match="invalid argument"):
            m.write(str(tmp_path / "no such directory" / "map.ot"))


def test_set_leaves_and_query_refusals(fe):
    leaves = [l for n, l in PLANTED if n == "random 257"][0]
    with fe.octomap(300) as m:
        m.set_leaves(leaves[:100])
        twice = np.concatenate([leaves, leaves[200:201]])
        with pytest.raises(Exception, match="invalid argument.*repeated"):
            m.set_leaves(twice)
        assert len(m) == 0 and len(m.leaves()) == 0 and len(m.tree()) == 0  # left empty
        m.set_leaves(leaves[:100])
        with pytest.raises(Exception, match="capacity"):
            m.set_leaves(np.concatenate([leaves, to.random_leaves(1025, 5)[:44]]))  # 301 > 300
        same(m.leaves(), oo.records([(oo.pack(*l["key"]), l["log_odds"], tuple(l["rgb"])) for l in leaves[:100]]), "unchanged")
        bad = leaves[:4].copy()
        bad["zero1"][2] = 1
        with pytest.raises(Exception, match="invalid argument.*padding"):
            m.set_leaves(bad)
        assert len(m) == 0
        bad = leaves[:4].copy()
        bad["log_odds"][1] = np.inf
        with pytest.raises(Exception, match="invalid argument"):
            m.set_leaves(bad)
        m.set_leaves(leaves)
        for depth, thr in ((-1, 0.0), (17, 0.0), (3, float("nan"))):
            with pytest.raises(Exception, match="invalid argument"):
                m.nodes_at_depth(depth, thr)
