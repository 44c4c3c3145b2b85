"""-m gpu: the contract of the resident-node table ("The node table"), at the smallest sizes where it can break:
max_nodes = 3, max_keypoints = 64, nodes of 0 .. 8 random rows, through the four host upload calls (rgbdfe_upload_node,
rgbdfe_upload_nodes, rgbdfe_upload_sift_node, rgbdfe_upload_float_node), rgbdfe_release_node and rgbdfe_node_count.

  * a fresh id takes a free slot or the call is refused with RGBDFE_ERR_CAPACITY, leaving every resident node as it was
  * rgbdfe_upload_nodes is all-or-nothing: too many fresh ids, or an id listed twice, and nothing of the call happened
  * a resident id is rewritten in its own slot, whatever kind it had and gets
  * release / upload cycles never lose a slot

(With max_nodes = 3 a list of four distinct ids never fits, so the all-or-nothing case has its refused call with four ids,
two of them resident, and its accepted call with three, two of them resident.)"""
import numpy as np
import pytest

from rgbdslam_v2_amd._lib import RgbdfeError

pytestmark = pytest.mark.gpu

MAX_NODES, MAX_KP = 3, 64
NO_SLOT = r"^capacity exceeded: no free node slot \(max_nodes\)"
TWICE = r"^invalid argument: a node id appears twice"


@pytest.fixture()
def fe():
    from rgbdslam_v2_amd.frontend import FrontEnd
    f = FrontEnd(device_id=0, max_nodes=MAX_NODES, max_keypoints=MAX_KP, max_pairs_per_batch=8)
    yield f
    f.close()


def _xyz(rng, n):
    p = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    p[:, 2] += 2.5
    p[:, 3] = 1
    return p


def _orb(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8), _xyz(rng, n)


def _flt(rng, n):
    return rng.uniform(0, 0.4, (n, 128)).astype(np.float32), _xyz(rng, n)


# the four upload calls as (node id, row count) -> None
UPLOADS = {
    "upload_node": lambda fe, rng, i, n: fe.upload_node(i, *_orb(rng, n)),
    "upload_nodes": lambda fe, rng, i, n: fe.upload_nodes([i], *[[a] for a in _orb(rng, n)]),
    "upload_sift_node": lambda fe, rng, i, n: fe.upload_sift_node(i, *_flt(rng, n)),
    "upload_float_node": lambda fe, rng, i, n: fe.upload_float_node(i, *_flt(rng, n)),
}
KINDS = list(UPLOADS)


def _counts(fe, ids):
    return [fe.node_count(i) for i in ids]


def test_a_full_table_refuses_a_fourth_id_in_every_upload_call(fe):
    rng = np.random.default_rng(1)
    want = {10: 8, 11: 3, 12: 5}
    for (i, n), kind in zip(want.items(), ("upload_node", "upload_sift_node", "upload_float_node")):
        UPLOADS[kind](fe, rng, i, n)
    assert _counts(fe, want) == list(want.values())
    for kind in KINDS:
        with pytest.raises(RgbdfeError, match=NO_SLOT):
            UPLOADS[kind](fe, rng, 13, 4)
        assert fe.node_count(13) < 0, kind
        assert _counts(fe, want) == list(want.values()), kind


def test_upload_nodes_is_all_or_nothing_on_capacity(fe):
    rng = np.random.default_rng(2)
    d1, x1 = _orb(rng, 8)
    d2, x2 = _orb(rng, 6)
    fe.upload_nodes([1, 2], [d1, d2], [x1, x2])
    before = fe.match_pair_list([2], [1]).tobytes()
    new = [_orb(rng, n) for n in (7, 1, 5, 2)]
    d, x = [a for a, _ in new], [b for _, b in new]
    with pytest.raises(RgbdfeError, match=NO_SLOT):          # two resident, two fresh, one free slot
        fe.upload_nodes([1, 5, 2, 6], d, x)
    assert _counts(fe, [1, 2]) == [8, 6] and fe.node_count(5) < 0 and fe.node_count(6) < 0
    assert fe.match_pair_list([2], [1]).tobytes() == before  # the residents' rows are what they were
    fe.upload_nodes([1, 5, 2], d[:3], x[:3])                 # two resident, one fresh: fits
    assert _counts(fe, [1, 5, 2]) == [7, 1, 5]
    with pytest.raises(RgbdfeError, match=NO_SLOT):
        fe.upload_node(6, *_orb(rng, 2))


def test_upload_nodes_refuses_an_id_listed_twice_and_changes_nothing(fe):
    rng = np.random.default_rng(3)
    fe.upload_node(1, *_orb(rng, 8))
    fe.upload_node(2, *_orb(rng, 4))
    before = fe.match_pair_list([1], [2]).tobytes()
    new = [_orb(rng, n) for n in (3, 2, 5)]
    for ids in ([1, 7, 7], [7, 1, 7], [1, 1, 7]):
        with pytest.raises(RgbdfeError, match=TWICE):
            fe.upload_nodes(ids, [a for a, _ in new], [b for _, b in new])
        assert _counts(fe, [1, 2]) == [8, 4] and fe.node_count(7) < 0
        assert fe.match_pair_list([1], [2]).tobytes() == before
    fe.upload_node(7, *_orb(rng, 1))                         # the free slot is still there
    assert fe.node_count(7) == 1


def test_a_resident_id_keeps_its_slot_through_every_kind(fe):
    from rgbdslam_v2_amd.frontend import FrontEnd
    rng = np.random.default_rng(4)
    fd, fx = _flt(rng, 6)
    od, ox = _orb(rng, 7)
    fe.upload_node(1, *_orb(rng, 8))
    fe.upload_float_node(1, fd, fx)
    assert fe.node_count(1) == 6
    fe.upload_sift_node(1, *_flt(rng, 0))
    assert fe.node_count(1) == 0
    fe.upload_sift_node(1, *_flt(rng, 5))
    assert fe.node_count(1) == 5
    fe.upload_node(1, od, ox)
    assert fe.node_count(1) == 7
    # the other two slots are still free, and no more than those two
    od2, ox2 = _orb(rng, 8)
    gd, gx = _flt(rng, 8)
    fe.upload_nodes([2], [od2], [ox2])
    fe.upload_float_node(3, gd, gx)
    for kind in KINDS:
        with pytest.raises(RgbdfeError, match=NO_SLOT):
            UPLOADS[kind](fe, rng, 4, 1)
    assert _counts(fe, [1, 2, 3]) == [7, 8, 8]
    # the rewritten slot holds what a fresh context holds: the ORB pair, then (1 a float node again) the FLANN pair
    orb_pair = fe.match_pair_list([1], [2])
    fe.upload_float_node(1, fd, fx)
    recs, dist = fe.match_flann_pair_list([1], [3])
    other = FrontEnd(device_id=0, max_nodes=MAX_NODES, max_keypoints=MAX_KP, max_pairs_per_batch=8)
    try:
        other.upload_node(1, od, ox)
        other.upload_node(2, od2, ox2)
        assert other.match_pair_list([1], [2]).tobytes() == orb_pair.tobytes()
        other.upload_float_node(1, fd, fx)
        other.upload_float_node(3, gd, gx)
        r2, d2 = other.match_flann_pair_list([1], [3])
        n = int(recs["n_all"][0])
        assert n == r2["n_all"][0] and np.array_equal(recs["all_q"][0][:n], r2["all_q"][0][:n])
        assert np.array_equal(recs["all_t"][0][:n], r2["all_t"][0][:n]) and np.array_equal(dist[0][:n], d2[0][:n])
    finally:
        other.close()


def test_release_and_refill_cycles_never_lose_a_slot(fe):
    rng = np.random.default_rng(5)
    live = {}
    for i in range(MAX_NODES):
        live[i] = int(rng.integers(0, 9))
        UPLOADS[KINDS[i % 4]](fe, rng, i, live[i])
    for cycle in range(3 * MAX_NODES):
        new = 100 + cycle
        with pytest.raises(RgbdfeError, match=NO_SLOT):      # full before ...
            UPLOADS[KINDS[(cycle + 1) % 4]](fe, rng, new, 2)
        gone = sorted(live)[0]
        fe.release_node(gone)
        del live[gone]
        assert fe.node_count(gone) < 0
        live[new] = int(rng.integers(0, 9))
        UPLOADS[KINDS[cycle % 4]](fe, rng, new, live[new])   # ... and one slot, no more, after the release
        keep = sorted(live)[0]                                # a resident id rewritten with another kind: no slot taken
        live[keep] = int(rng.integers(0, 9))
        UPLOADS[KINDS[(cycle + 2) % 4]](fe, rng, keep, live[keep])
        assert _counts(fe, live) == list(live.values()), cycle
    for i in list(live):                                      # all three slots come back
        fe.release_node(i)
    for i in range(MAX_NODES):
        fe.upload_node(200 + i, *_orb(rng, 8))
    assert _counts(fe, [200, 201, 202]) == [8, 8, 8]


@pytest.mark.parametrize("kind", KINDS)
def test_an_empty_upload_makes_a_resident_node_of_no_rows(fe, kind):
    rng = np.random.default_rng(6)
    assert fe.node_count(9) < 0
    UPLOADS[kind](fe, rng, 9, 0)
    assert fe.node_count(9) == 0
    UPLOADS[kind](fe, rng, 9, 8)                             # ... which an upload rewrites in place
    assert fe.node_count(9) == 8
    UPLOADS[kind](fe, rng, 9, 0)
    assert fe.node_count(9) == 0
    fe.release_node(9)
    assert fe.node_count(9) < 0
