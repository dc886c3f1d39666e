"""Inputs shared by the marker-build tests (tests/test_gpu_marker_build.py, tests/test_gpu_build_markers.py): three documents and, per window, site
records at every edge of the window rule.  numpy on the CPU from a fixed seed; no device."""
import numpy as np

import marker_build_model as MB

ACGT = np.frombuffer(b"ACGT", np.uint8)
DOC_LENS = (150, 97, 131)


def edge_text():
    rng = np.random.default_rng(19)
    return np.frombuffer(b"#".join(rng.choice(ACGT, k).tobytes() for k in DOC_LENS) + b"\x01", np.uint8).copy()


def edge_records(w):
    """per document: sites at 0, w - 2, w - 1 and the last base (the last document's right before the terminator), and in the first a stretch of w + 3
    consecutive sites; alleles 0 and 15 and contig bits, so that the order of the values is not the order of the positions"""
    starts = np.cumsum((0,) + tuple(k + 1 for k in DOC_LENS))[:-1].tolist()
    docs = []
    for d, (s, k) in enumerate(zip(starts, DOC_LENS)):
        offs = {0, max(w - 2, 0), w - 1, k - 1}
        if d == 0:
            offs |= set(range(70, 70 + w + 3))
        offs = sorted(o for o in offs if o < k)
        docs.append((s, [(o, MB.marker_value(15 if (o * 7 + d) % 3 == 0 else 0, (4095 - o * 5) % 4096 if o % 2 else d, o)) for o in offs]))
    return MB.records(docs, w)
