"""Generates tests/golden/flow_decode.npz: what the REFERENCE's decode_flow (utils/general_utils.py) returns on the designed codes of
tests/flow_ref.py and on a sweep of the 16-bit range, captured by importing the reference's module on the CPU with a stub standing in
for cv2 (decode_flow itself is numpy only).  The fixture holds arrays only: the codes, the decoded flow, the mask.

Run:  python tools/make_golden_flow_decode.py <path of the reference checkout>
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import flow_ref as fr  # noqa: E402


def codes():
    """uint16 [n,1,3]: the designed pixels, then every 251st code in u with the mirrored code in v, both sides of the validity threshold."""
    sweep = np.arange(0, 65536, 251, dtype=np.int64)
    rows = list(fr.DESIGNED_CODES) + [(int(c), int(65535 - c), 32768 + (i % 3) - 1) for i, c in enumerate(sweep)]
    return np.array(rows, np.uint16).reshape(-1, 1, 3)


def main(reference):
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, reference)
    from utils.general_utils import decode_flow
    enc = codes()
    flow, mask = decode_flow(enc)
    assert flow.dtype == np.float32 and mask.dtype == np.float32 and flow.shape == enc.shape[:2] + (2,)
    out = os.path.join(ROOT, "tests", "golden", "flow_decode.npz")
    np.savez(out, codes=enc, flow=flow, mask=mask)
    print(out, enc.shape, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
