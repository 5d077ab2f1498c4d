"""Writes tests/golden/resize.npz with Pillow (12.2.0 when this was last run): for the named cases of tests/resize_cases.py, seeded
random bytes and the saturating 0 / 255 pattern, and Pillow's Image.resize of both for bilinear, box and bicubic; and five small frames
with their bilinear resize for the FrameStore / FrameStream tests.

    python tests/golden/make_golden_resize.py

Keys: "<case>/<content>/in", "<case>/<content>/<filter>", "frames/in" [5,15,23,3], "frames/out" [5,7,11,3], "pillow" (its version)."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_cases as rc                                   # noqa: E402

RESAMPLE = {"bilinear": 2, "bicubic": 3, "box": 4}


def pil_resize(a, out_hw, resample):
    return np.asarray(Image.fromarray(a).resize((out_hw[1], out_hw[0]), resample=RESAMPLE[resample]))


def main():
    out = {"pillow": np.array(PIL.__version__)}
    for case in rc.NAMED:
        H_in, W_in, H_out, W_out = case
        for content, make in rc.CONTENT.items():
            a = make(H_in, W_in)
            out[f"{rc.case_id(case)}/{content}/in"] = a
            for f in rc.FILTERS:
                out[f"{rc.case_id(case)}/{content}/{f}"] = pil_resize(a, (H_out, W_out), f)
    frames = np.stack([rc.random_bytes(15, 23, seed=100 + i) for i in range(5)])
    out["frames/in"] = frames
    out["frames/out"] = np.stack([pil_resize(f, (7, 11), "bilinear") for f in frames])
    path = os.path.join(HERE, "resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
