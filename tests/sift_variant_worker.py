"""Worker of tests/test_gpu_sift_variants.py: python sift_variant_worker.py OUT.npz

The switches that choose the SIFT dot kernel (RGBDFE_SIFT_ONEPASS, RGBDFE_SIFT_ROWS64, RGBDFE_SIFT_FAST_KEYS) are read once
per process, so every setting gets a process of its own.  The worker builds the fixed case list of
sift_match_reference.worker_cases() and the mixed batch from their seeds, runs them through one FrontEnd and writes the
raw match lists and records to OUT.npz; the parent compares them with the oracle.  Exit status 3: one of the worker's own
sanity assertions failed (the message is on stderr); any other non-zero status is a crash."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for p in (_HERE, os.path.dirname(_HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import sift_match_reference as sr  # noqa: E402

FRONT_END = dict(device_id=0, max_nodes=12, max_keypoints=1536, max_pairs_per_batch=64)


def run(out_path):
    from rgbdslam_v2_amd.frontend import FrontEnd
    fe = FrontEnd(**FRONT_END)
    res = {}
    try:
        for c in sr.worker_cases():
            fe.upload_sift_node(1, c["d1"], c["xyz1"])
            fe.upload_sift_node(2, c["d2"], c["xyz2"])
            mq, mt, md = fe.sift_match_nodes(1, 2)
            assert len(mq) == len(mt) == len(md) <= len(c["d1"]), c["name"]
            res[c["name"] + "/q"], res[c["name"] + "/t"], res[c["name"] + "/d"] = mq, mt, md
        fe.release_node(1)
        fe.release_node(2)
        nodes, pq, pt = sr.mixed_batch_nodes()
        for f, (d, x) in enumerate(nodes):
            fe.upload_sift_node(f, d, x)
        out, dist = fe.match_sift_pair_list(pq, pt)
        assert len(out) == len(pq)
        res["mixed/records"] = np.frombuffer(out.tobytes(), np.uint8)
        res["mixed/dist"] = np.asarray(dist)
    finally:
        fe.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    try:
        run(sys.argv[1])
    except AssertionError as e:
        sys.stderr.write("worker assertion: %r\n" % (e,))
        sys.exit(3)
    print("worker ok")
