"""-m gpu: the 512-query Hamming kernel on 16x16x128 fp4 tiles (hamming_mfma_x16_kernel) against the popcount kernel
(mode 0), bit for bit, on and around every boundary of its blocks, query tiles, 16-row sub-tiles and stages; the dispatch
that picks a tile shape for large batches only; and the shape in the graph cache's key.  Integer work: keys are equal or
wrong."""
import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

# The MFMA tile a new context gives the 512-query blocks of a large batch: the form measured faster at the headline batch
# (profiles/hamming_x16_95ed2de.json).
DEFAULT_WIDE_SHAPE = 16

# query counts: the grid of test_gpu_hamming_wide.py (a 32-query operand tile, a wave of 128, 256, a block of 512, two
# blocks) and one 16-query tile of the small MFMA
NQ = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000]
# train counts (nt rows are nt - 1 candidates): the grid of test_gpu_hamming_wide.py (nothing searchable, a ragged tile
# alone, a full tile alone, a full tile + one row, one stage, two stages with two slots to spare, eight stages) and ragged
# tiles that end with the first 16-row half or one row into the second: 16 and 17 candidates alone (nt 17, 18), and
# behind a full tile (nt 49, 50)
NT = [1, 2, 17, 18, 33, 34, 49, 50, 129, 162, 1000]


@pytest.fixture(scope="module")
def ctxs():
    """x16: a context at the default mode (3) whose blocks are 512 queries whatever the batch and whose tile is 16x16x128;
    ref: the popcount kernel."""
    import os
    from rgbdslam_v2_amd.frontend import FrontEnd
    saved = {k: os.environ.get(k) for k in ("RGBDFE_HAMMING_WIDE", "RGBDFE_HAMMING_MODE", "RGBDFE_HAMMING_SHAPE")}
    os.environ["RGBDFE_HAMMING_WIDE"] = "1"
    os.environ.pop("RGBDFE_HAMMING_MODE", None)
    os.environ.pop("RGBDFE_HAMMING_SHAPE", None)
    try:
        x16 = FrontEnd(device_id=0, max_nodes=8, max_keypoints=1024, max_pairs_per_batch=64)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    x16.set_hamming_shape(16)
    ref = FrontEnd(device_id=0, max_nodes=8, max_keypoints=1024, max_pairs_per_batch=64)
    ref.set_hamming_mode(0)
    yield x16, ref
    x16.close()
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
    x16, ref = ctxs
    got = x16.bruteForceSearchORB_batch(q, t)
    assert x16.hamming_wide_last == 1 and x16.hamming_shape_last == 16
    want = ref.bruteForceSearchORB_batch(q, t)
    assert ref.hamming_wide_last == 0 and ref.hamming_shape_last == 0
    return got, want


@pytest.mark.parametrize("nt", NT)
def test_x16_kernel_equals_popcount_kernel(ctxs, pool, nt):
    q, t = pool
    for nq in NQ:
        # the train rows are taken from the END of the pool for odd query counts: other rows in the ragged tile
        tt = t[:nt] if nq % 2 == 0 else t[1000 - nt:]
        (hd, idx), (hd0, idx0) = both(ctxs, q[:nq], tt)
        assert np.array_equal(hd, hd0), (nq, nt)
        assert np.array_equal(idx, idx0), (nq, nt)
        if nt == 1:
            assert np.all(hd == 257) and np.all(idx == -1)   # features.cpp:172-173: nothing was searched


def test_x16_kernel_equals_the_oracle_at_the_headline_shape(ctxs, pool):
    q, t = pool
    (hd, idx), _ = both(ctxs, q, t)
    hd2, idx2 = po.hamming_nn_batch(q, t)
    assert np.array_equal(hd, hd2) and np.array_equal(idx, idx2)


@pytest.mark.parametrize("nq,nt", [(513, 129), (1000, 1000), (257, 34), (17, 50)])
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


@pytest.mark.parametrize("nt", [2, 18, 33, 34, 50, 129, 1000])
def test_identical_and_complementary_descriptors(ctxs, nt):
    """Every train row is the same descriptor r: a query equal to r has hd = 0, its complement hd = 256, both at row 0 --
    no later copy, no row seen a second time in a slot without a tile of its own, and none of the rows that do not take
    part, may win."""
    rng = np.random.default_rng(nt)
    r = rng.integers(0, 256, 32, dtype=np.uint8)
    t = np.repeat(r[None, :], nt, axis=0)
    q = np.repeat(r[None, :], 515, axis=0)
    q[1::2] = ~q[1::2]
    (hd, idx), (hd0, idx0) = both(ctxs, q, t)
    assert np.array_equal(hd, hd0) and np.array_equal(idx, idx0)
    assert np.all(hd[0::2] == 0) and np.all(hd[1::2] == 256) and np.all(idx == 0)


@pytest.mark.parametrize("nt", [2, 17, 18, 33, 34, 40, 49, 50, 129, 1000])
def test_the_last_train_row_is_never_a_candidate(ctxs, pool, nt):
    """features.cpp:174 searches rows [0, nt - 1).  Queries that EQUAL the last row (and the rows behind it in the node's
    last tile, which the kernel overwrites in LDS) must come back with their best match among the rows in front."""
    q, t = pool
    tt = t[:nt].copy()
    qq = q[:300].copy()
    qq[::3] = tt[nt - 1]
    (hd, idx), (hd0, idx0) = both(ctxs, qq, tt)
    assert np.array_equal(hd, hd0) and np.array_equal(idx, idx0)
    hd2, idx2 = po.hamming_nn_batch(qq, tt)
    assert np.array_equal(hd, hd2) and np.array_equal(idx, idx2)
    assert np.all(idx < nt - 1)


def test_dispatch_and_the_shape_in_the_graph_key(monkeypatch):
    """A new context with nothing forced: 3840 pairs of up to 1000 keypoints are 512-query blocks on the measured winner's
    tile, 20 pairs are today's 256-query kernel (32x32x64).  With graph capture on, as bench.py runs, a batch of the SAME
    geometry after set_hamming_shape is captured anew (rgbdfe_graph_stats) -- under a key without the shape it would replay
    the first kernel's graph -- and going back replays the first graphs.  Every form gives the pairs mode 0 gives."""
    import torch
    from rgbdslam_v2_amd._lib import RESULT_DTYPE, RgbdfeError
    from rgbdslam_v2_amd.frontend import FrontEnd
    for k in ("RGBDFE_HAMMING_WIDE", "RGBDFE_HAMMING_MODE", "RGBDFE_HAMMING_SHAPE"):
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(77)
    rows = [1000, 999, 993, 961, 960, 513, 512, 511, 257, 256, 129, 34, 33, 32, 2, 1, 1000, 777, 640, 300]
    n_nodes = len(rows)
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in rows]
    for k in range(1, n_nodes):   # related nodes: matches below the distance threshold, and ties
        m = min(rows[k], rows[0])
        take = rng.permutation(m)[: m // 2]
        descs[k][take] = descs[0][take]
        descs[k][take] ^= np.packbits(rng.random((len(take), 256)) < 0.04, axis=1, bitorder="little")
    xyzs = [np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(1, 3, (n, 1)), np.ones((n, 1))], 1).astype(np.float32)
            for n in rows]
    n_pairs = 3840
    pq = rng.integers(0, n_nodes, n_pairs).astype(np.int32)
    pt = ((pq + 1 + rng.integers(0, n_nodes - 1, n_pairs)) % n_nodes).astype(np.int32)
    pq[0], pt[0] = 0, 16   # 1000 x 1000 is in the batch

    def big_batch(fe, buf):
        # (one batch on one lane, as bench.py submits them: match_pair_list would cut a long list into one piece per lane;
        # the output buffer is part of a cached graph's key, so a context keeps one)
        fe.wait_ticket(fe.submit_pair_list(pq, pt, buf.data_ptr()), None)
        return np.frombuffer(buf.cpu().numpy().tobytes(), RESULT_DTYPE)

    def moved(fe, before):
        now = fe.graph_stats()
        return {k: now[k] - before[k] for k in ("captures", "launches", "cached", "plain_batches", "capture_failures")}

    other = 48 - DEFAULT_WIDE_SHAPE
    outs = {}
    for mode in (None, 0):
        fe = FrontEnd(device_id=0, max_nodes=32, max_keypoints=1024, max_pairs_per_batch=4096)
        if mode is not None:
            fe.set_hamming_mode(mode)
        else:
            fe.set_graph_capture(True)               # the path bench.py runs: cached hipGraphs of whole batches
        for k in range(n_nodes):
            fe.upload_node(k, descs[k], xyzs[k])
        buf = torch.zeros(n_pairs * RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        assert fe.hamming_shape_last == -1
        st = fe.graph_stats()
        big = big_batch(fe, buf)
        seen = [(fe.hamming_wide_last, fe.hamming_shape_last)]
        if mode is None:
            assert st["enabled"] == 1 and moved(fe, st) == {"captures": 1, "launches": 1, "cached": 1, "plain_batches": 0,
                                                            "capture_failures": 0}
        outs[mode] = [big]
        if mode is None:
            # A cached graph also belongs to one slot of the context's ring of batch buffers, so the same batch is captured
            # once per slot before it comes back as a replay.  `ring` = the batches until the first replay; from then on
            # `ring` batches in a row visit every slot once, wherever the ring stands.
            ring = 1
            while True:
                before = fe.graph_stats()
                outs[mode].append(big_batch(fe, buf))
                d = moved(fe, before)
                assert d["launches"] == 1 and d["plain_batches"] == 0 and d["capture_failures"] == 0, d
                if d["captures"] == 0:               # the same batch again: a replay of a cached graph
                    assert d["cached"] == 0
                    break
                ring += 1
                assert ring <= 8
        small = fe.match_pair_list(pq[:20], pt[:20])
        seen.append((fe.hamming_wide_last, fe.hamming_shape_last))
        outs[mode].insert(1, small)
        if mode is None:
            assert seen == [(1, DEFAULT_WIDE_SHAPE), (0, 32)], seen
            big_batch(fe, buf)
            assert fe.hamming_shape_last == DEFAULT_WIDE_SHAPE

            def turn():
                before = fe.graph_stats()
                for _ in range(ring):
                    outs[mode].append(big_batch(fe, buf))
                return moved(fe, before)

            replay = {"captures": 0, "launches": ring, "cached": 0, "plain_batches": 0, "capture_failures": 0}
            fresh = {"captures": ring, "launches": ring, "cached": ring, "plain_batches": 0, "capture_failures": 0}
            assert turn() == replay                  # every slot has its graph of the default shape
            fe.set_hamming_shape(other)
            assert turn() == fresh                   # same geometry, the other kernel: NOT a replay of the first graphs
            assert (fe.hamming_wide_last, fe.hamming_shape_last) == (1, other)
            assert turn() == replay
            fe.match_pair_list(pq[:20], pt[:20])     # small batches do not care
            assert (fe.hamming_wide_last, fe.hamming_shape_last) == (0, 32)
            fe.set_hamming_shape(0)
            assert turn() == replay                  # the first graphs again
            assert fe.hamming_shape_last == DEFAULT_WIDE_SHAPE
            with pytest.raises(RgbdfeError):
                fe.set_hamming_shape(8)
            fe.set_hamming_mode(4)                   # mode 4 by name is the 32x32x64 kernel whatever the shape
            fe.set_hamming_shape(16)
            assert turn() == fresh                   # (the mode is in the key as well)
            assert (fe.hamming_wide_last, fe.hamming_shape_last) == (1, 32)
        else:
            assert seen == [(0, 0), (0, 0)], seen
            assert moved(fe, st) == {"captures": 0, "launches": 0, "cached": 0, "plain_batches": 0, "capture_failures": 0}
        fe.close()
    want_big, want_small = outs[0]
    assert len(outs[None]) > 2 + 6
    for f in ("n_all", "all_q", "all_t", "all_hd"):
        assert np.array_equal(outs[None][1][f], want_small[f]), f
        for k in [0] + list(range(2, len(outs[None]))):
            assert np.array_equal(outs[None][k][f], want_big[f]), (f, k)
    assert want_big["n_all"].max() > 50
