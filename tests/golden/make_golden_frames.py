"""Captures tests/golden/frames.npz from the reference checkout: the float ground-truth image the reference's OWN loader makes of a
decoded 8-bit frame.

    python tests/golden/make_golden_frames.py /path/to/reference

Nothing of the reference is copied: utils/general_utils.py is imported for PILtoTorch (its third-party imports stubbed, as
make_golden.py does), and `im_reader` is cut out of scene/__init__.py at capture time -- from its `def` line to its `return` --
dedented, compiled and executed with `Image.open` handing back the seeded PIL image.  Runs on the CPU.  Recorded, for an RGB
[53,139,3] and an RGBA [53,139,4] image that each hold all 256 byte values: the uint8 input and, for im_scale 1.0, 0.5 and 1.7, the
float32 [3,H,W] tensor im_reader returns (not contiguous there: stride (1, 3W, 3) for both; stored as numpy stores it).
"""
import os
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "frames.npz")
H, W = 53, 139
SCALES = (1.0, 0.5, 1.7)


def reference_reader(ref):
    for name in ("cv2",):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, ref)
    from utils.general_utils import PILtoTorch
    lines = open(os.path.join(ref, "scene", "__init__.py")).read().splitlines()
    start = [i for i, l in enumerate(lines) if l.strip().startswith("def im_reader(")]
    assert start, "anchor `def im_reader(` not found in the reference's scene/__init__.py"
    blocks = set()                                   # (the train- and the test-camera getter each define it: the same text)
    for s0 in start:
        end = [i for i, l in enumerate(lines) if i > s0 and l.strip().startswith("return ")]
        assert end, "im_reader's return not found"
        blocks.add(textwrap.dedent("\n".join(lines[s0:end[0] + 1])))
    assert len(blocks) == 1, "the reference's im_reader definitions differ"
    block = blocks.pop()
    assert "PILtoTorch" in block and "im_scale" in block and "clamp" in block
    return PILtoTorch, compile(block, "reference_scene_im_reader", "exec")


def image(seed, channels):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, size=(H, W, channels), dtype=np.uint8)
    for c in range(channels):                                                      # every byte value in every channel
        a[c, :256 // 2, c] = np.arange(0, 256, 2, dtype=np.uint8)
        a[-1 - c, :256 // 2, c] = np.arange(1, 256, 2, dtype=np.uint8)
    assert all(len(np.unique(a[..., c])) == 256 for c in range(channels))
    return a


def main():
    from PIL import Image
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("EX4D_REFERENCE", "")
    assert ref and os.path.exists(os.path.join(ref, "scene", "__init__.py")), "usage: make_golden_frames.py <reference checkout>"
    PILtoTorch, code = reference_reader(ref)
    torch.set_num_threads(1)
    out = {"im_scales": np.array(SCALES, np.float64)}
    for tag, seed, channels, mode in (("rgb", 41, 3, "RGB"), ("rgba", 42, 4, "RGBA")):
        u8 = image(seed, channels)
        pil = Image.fromarray(u8, mode)
        # PILtoTorch resizes to the resolution it is given; at the image's own size PIL hands the bytes back
        assert np.array_equal(np.array(pil.resize((W, H), resample=2)), u8), "PIL's same-size resize changed the bytes"
        env = {"PILtoTorch": PILtoTorch, "Image": types.SimpleNamespace(open=lambda path, pil=pil: pil), "ImageFile": types.SimpleNamespace()}
        exec(code, env)
        out[tag + "_u8"] = u8
        for k, im_scale in enumerate(SCALES):
            t = env["im_reader"]("frame.png", (W, H), im_scale)
            assert t.dtype == torch.float32 and tuple(t.shape) == (3, H, W) and t.stride() == (1, 3 * W, 3)
            out[f"{tag}_f32_{k}"] = t.numpy()
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
