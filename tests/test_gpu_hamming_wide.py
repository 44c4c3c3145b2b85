"""-m gpu: the pipelined fp4 Hamming kernel with four query tiles per wave (512 queries per block, Hamming mode 4) against
the popcount kernel (mode 0), bit for bit, on and around every boundary of its blocks, tiles and stages; and the dispatch
that picks it for large batches only.  Integer work: keys are equal or wrong."""
import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

# query counts: one tile of 32, one wave (4 tiles = 128), half a block (256 = today's block), a block (512), two blocks
NQ = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000]
# train counts (the last row is never searched: nt rows are nt - 1 candidates): nothing searchable; one candidate = a ragged
# tile alone; 32 = one full tile alone; 33 = a full tile + one ragged row; 128 = four full tiles = exactly one stage;
# 161 = five full tiles + a ragged row = two stages with two phantoms; 999 = 31 full tiles + 7 rows = eight full stages
NT = [1, 2, 33, 34, 129, 162, 1000]


@pytest.fixture(scope="module")
def ctxs():
    from rgbdslam_v2_amd.frontend import FrontEnd
    wide = FrontEnd(device_id=0, max_nodes=8, max_keypoints=1024, max_pairs_per_batch=64)
    wide.set_hamming_mode(4)
    ref = FrontEnd(device_id=0, max_nodes=8, max_keypoints=1024, max_pairs_per_batch=64)
    ref.set_hamming_mode(0)
    yield wide, ref
    wide.close()
    ref.close()


@pytest.fixture(scope="module")
def pool():
    """1000 train rows and 1000 query rows; two thirds of the queries are noisy copies of train rows, so that the nearest
    neighbours are spread over all tiles instead of sitting wherever chance puts a distance of ~100."""
    rng = np.random.default_rng(20260923)
    t = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    src = rng.integers(0, 1000, 1000)
    related = rng.random(1000) < 0.66
    flips = np.packbits(rng.random((1000, 256)) < 0.05, axis=1, bitorder="little")
    q[related] = t[src[related]] ^ flips[related]
    return q, t


def both(ctxs, q, t):
    wide, ref = ctxs
    got = wide.bruteForceSearchORB_batch(q, t)
    assert wide.hamming_wide_last == 1
    want = ref.bruteForceSearchORB_batch(q, t)
    assert ref.hamming_wide_last == 0
    return got, want


@pytest.mark.parametrize("nt", NT)
def test_wide_kernel_equals_popcount_kernel(ctxs, pool, nt):
    q, t = pool
    for nq in NQ:
        # the train rows are taken from the END of the pool for odd query counts: other rows in the ragged tile
        tt = t[:nt] if nq % 2 == 0 else t[1000 - nt:]
        (hd, idx), (hd0, idx0) = both(ctxs, q[:nq], tt)
        assert np.array_equal(hd, hd0), (nq, nt)
        assert np.array_equal(idx, idx0), (nq, nt)
        if nt == 1:
            assert np.all(hd == 257) and np.all(idx == -1)   # features.cpp:172-173: nothing was searched


def test_wide_kernel_equals_the_oracle_at_the_headline_shape(ctxs, pool):
    q, t = pool
    (hd, idx), _ = both(ctxs, q, t)
    hd2, idx2 = po.hamming_nn_batch(q, t)
    assert np.array_equal(hd, hd2) and np.array_equal(idx, idx2)


@pytest.mark.parametrize("nq,nt", [(513, 129), (1000, 1000), (257, 34)])
def test_planted_ties_first_row_wins(ctxs, nq, nt):
    rng = np.random.default_rng(nq * 31 + nt)
    base = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    t = base[rng.integers(0, 8, nt)]
    q = base[rng.integers(0, 8, nq)]
    (hd, idx), (hd0, idx0) = both(ctxs, q, t)
    assert np.array_equal(hd, hd0) and np.array_equal(idx, idx0)
    searched = t[:nt - 1]
    for k in range(0, nq, 37):
        same = np.flatnonzero((searched == q[k]).all(axis=1))
        if len(same):
            assert hd[k] == 0 and idx[k] == same[0]


@pytest.mark.parametrize("nt", [2, 33, 34, 129, 1000])
def test_identical_and_complementary_descriptors(ctxs, nt):
    """Every train row is the same descriptor r: a query equal to r has hd = 0, its complement hd = 256, both at row 0 --
    no later copy, and none of the rows that do not take part, may win."""
    rng = np.random.default_rng(nt)
    r = rng.integers(0, 256, 32, dtype=np.uint8)
    t = np.repeat(r[None, :], nt, axis=0)
    q = np.repeat(r[None, :], 515, axis=0)
    q[1::2] = ~q[1::2]
    (hd, idx), (hd0, idx0) = both(ctxs, q, t)
    assert np.array_equal(hd, hd0) and np.array_equal(idx, idx0)
    assert np.all(hd[0::2] == 0) and np.all(hd[1::2] == 256) and np.all(idx == 0)


@pytest.mark.parametrize("nt", [2, 33, 34, 40, 129, 1000])
def test_the_last_train_row_is_never_a_candidate(ctxs, pool, nt):
    """features.cpp:174 searches rows [0, nt - 1).  Queries that EQUAL the last row (and the rows behind it in the node's
    last tile, which the wide kernel overwrites in LDS) must come back with their best match among the rows in front."""
    q, t = pool
    tt = t[:nt].copy()
    qq = q[:300].copy()
    qq[::3] = tt[nt - 1]
    (hd, idx), (hd0, idx0) = both(ctxs, qq, tt)
    assert np.array_equal(hd, hd0) and np.array_equal(idx, idx0)
    hd2, idx2 = po.hamming_nn_batch(qq, tt)
    assert np.array_equal(hd, hd2) and np.array_equal(idx, idx2)
    assert np.all(idx < nt - 1)


def test_default_dispatch_takes_the_wide_kernel_for_large_batches_only(monkeypatch):
    """A new context (mode 3, block width chosen per batch): 3840 pairs of up to 1000 keypoints are 7680 blocks of 512 queries,
    ten per block slot of the chip, without train splits -- the wide kernel; 20 pairs split their train rows -- today's."""
    import torch
    from rgbdslam_v2_amd._lib import RESULT_DTYPE
    from rgbdslam_v2_amd.frontend import FrontEnd
    monkeypatch.delenv("RGBDFE_HAMMING_WIDE", raising=False)
    monkeypatch.delenv("RGBDFE_HAMMING_MODE", raising=False)
    rng = np.random.default_rng(77)
    rows = [1000, 999, 993, 961, 960, 513, 512, 511, 257, 256, 129, 34, 33, 32, 2, 1, 1000, 777, 640, 300]
    n_nodes = len(rows)
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in rows]
    for k in range(1, n_nodes):   # related nodes: matches below the distance threshold, and ties
        m = min(rows[k], rows[0])
        take = rng.permutation(m)[: m // 2]
        descs[k][take] = descs[0][take]
        descs[k][take] ^= np.packbits(rng.random((len(take), 256)) < 0.04, axis=1, bitorder="little")
    n_pairs = 3840
    pq = rng.integers(0, n_nodes, n_pairs).astype(np.int32)
    pt = ((pq + 1 + rng.integers(0, n_nodes - 1, n_pairs)) % n_nodes).astype(np.int32)
    pq[0], pt[0] = 0, 16   # 1000 x 1000 is in the batch
    outs = []
    for mode in (None, 0):
        fe = FrontEnd(device_id=0, max_nodes=32, max_keypoints=1024, max_pairs_per_batch=4096)
        if mode is not None:
            fe.set_hamming_mode(mode)
        for k in range(n_nodes):
            xyz = np.concatenate([rng.uniform(-1, 1, (rows[k], 2)), rng.uniform(1, 3, (rows[k], 1)),
                                  np.ones((rows[k], 1))], 1).astype(np.float32)
            fe.upload_node(k, descs[k], xyz)
        assert fe.hamming_wide_last == -1
        # (one batch on one lane, as bench.py submits them: match_pair_list would cut a long list into one piece per lane)
        buf = torch.zeros(n_pairs * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        fe.wait_ticket(fe.submit_pair_list(pq, pt, buf.data_ptr()), None)
        big = np.frombuffer(buf.cpu().numpy().tobytes(), RESULT_DTYPE)
        wide_big = fe.hamming_wide_last
        small = fe.match_pair_list(pq[:20], pt[:20])
        wide_small = fe.hamming_wide_last
        keys = [fe.hamming_nn_nodes(int(a), int(b)) for a, b in zip(pq[:6], pt[:6])]
        outs.append((big, small, keys))
        fe.close()
        assert (wide_big, wide_small) == ((1, 0) if mode is None else (0, 0)), mode
    for f in ("n_all", "all_q", "all_t", "all_hd"):
        assert np.array_equal(outs[0][0][f], outs[1][0][f]), f
        assert np.array_equal(outs[0][1][f], outs[1][1][f]), f
        assert np.array_equal(outs[0][0][f][:20], outs[0][1][f]), f   # and the same pairs, wide or not
    assert outs[0][0]["n_all"].max() > 50
    for (hd, idx), (hd0, idx0) in zip(outs[0][2], outs[1][2]):
        assert np.array_equal(hd, hd0) and np.array_equal(idx, idx0)


def test_mode_validation(ctxs):
    from rgbdslam_v2_amd._lib import RgbdfeError
    wide, _ = ctxs
    with pytest.raises(RgbdfeError):
        wide.set_hamming_mode(5)
    with pytest.raises(RgbdfeError):
        wide.set_hamming_mode(-1)
    wide.set_hamming_mode(4)
    assert wide.hamming_mode == 4
