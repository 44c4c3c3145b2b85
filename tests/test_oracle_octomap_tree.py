"""The two formulations of the tree of a leaf set in tests/octomap_tree_oracle.py agree byte for byte, and the independent
reader turns every written file back into the leaves (no GPU)."""
import numpy as np
import pytest

import octomap_oracle as oo
import octomap_tree_oracle as to

CASES = oo.cases()
PLANTED = to.planted_sets()


def check(leaves, resolution):
    lit = to.LiteralTree(leaves)
    rec, levels = to.flat_tree(leaves)
    want = lit.records()
    assert rec.dtype == to.NODE and rec.itemsize == 8
    assert rec.tobytes() == want.tobytes()
    for d in (0, 1, 8, 15, 16):
        assert levels[d].tobytes() == lit.at_depth(d).tobytes(), d
    blob = to.ot_file(want, resolution)
    rid, size, res, back = to.read_ot(blob)
    assert (rid, size, res) == ("ColorOcTree", len(want), "%g" % resolution)
    ref = leaves[np.argsort(leaves["key"][:, 0].astype(np.int64) | (leaves["key"][:, 1].astype(np.int64) << 16) |
                            (leaves["key"][:, 2].astype(np.int64) << 32))]
    assert back.tobytes() == ref.tobytes()
    return want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_formulations_agree_on_every_family(case):
    m = oo.run(case)
    leaves = m.leaves()
    rec = check(leaves, m.res)
    assert (len(rec) == 0) == (len(leaves) == 0)


@pytest.mark.parametrize("name,leaves", PLANTED, ids=[p[0] for p in PLANTED])
def test_formulations_agree_on_the_planted_sets(name, leaves):
    check(leaves, 0.05)


def planted(name):
    return [l for n, l in PLANTED if n == name][0]


def test_planted_sets_show_their_rule():
    """What each planted set is there for, stated on the literal tree's records."""
    one = to.LiteralTree(planted("one leaf")).records()
    assert len(one) == 17 and one["children"][16] == 0
    assert all(bin(int(m)).count("1") == 1 for m in one["children"][:16])
    sib = to.LiteralTree(planted("eight siblings")).records()
    assert len(sib) == 16 + 8 and sib["children"][15] == 0xff
    src = planted("eight siblings")
    col = src["rgb"][np.any(src["rgb"] != 255, axis=1)].astype(int)
    assert len(col) == 6 and np.any(col.sum(0) % 6 != 0)
    assert tuple(sib["rgb"][15]) == tuple(col.sum(0) // 6)
    hier = to.LiteralTree(planted("hierarchical average")).records()
    assert tuple(hier["rgb"][0]) == (100, 50, 0)  # ((1 + 2 + 2) // 3 + 200) // 2, not (1 + 2 + 2 + 200) // 4 = 51
    neg = to.LiteralTree(planted("negative only")).records()
    assert neg["log_odds"][0] == np.float32(-0.4) and np.all(neg["log_odds"] < 0)
    white = to.LiteralTree(planted("white subtree")).records()
    # the root's colour is the coloured depth-15 node's alone: the white sibling subtree does not halve it
    assert tuple(white["rgb"][0]) == ((90 + 31) // 2, (60 + 61) // 2, (31 + 90) // 2)
    far = to.LiteralTree(planted("root only shared")).records()
    # the extreme corners of the key space: two leaves under each of the root's children 0 and 7, apart from depth 2 on
    assert len(far) == 1 + 2 + 4 * 15 and far["children"][0] == 0x81 and far["log_odds"][0] == np.float32(2.0)
    assert far["children"][1] == 0x81 and far["children"][2] == 0x01


def test_reader_refuses_what_is_malformed():
    rec = to.LiteralTree(planted("eight siblings")).records()
    good = to.ot_file(rec, 0.05)
    to.read_ot(good)
    with pytest.raises(ValueError, match="truncated"):
        to.read_ot(good[:-8])
    with pytest.raises(ValueError, match="size"):
        to.read_ot(good.replace(b"size 24", b"size 23"))
    pruned = rec.copy()
    pruned["children"][15] = 0
    with pytest.raises(ValueError, match="pruned"):
        to.read_ot(to.ot_file(pruned[:16], 0.05))
