"""The resize cases the CPU and GPU tests share, and the mirror of include/ex4d_loss.h's EX4D_RESIZE_* tiling constants
(tests/test_cpu_resize.py parses the header and holds the two equal)."""
import numpy as np

# EX4D_RESIZE_* of include/ex4d_loss.h: name -> (value, the axis it tiles)
TILING = {
    "EX4D_RESIZE_H_PIXELS": (64, "W_out"),         # horizontal pass: output pixels of a workgroup's tile row
    "EX4D_RESIZE_H_ROWS": (4, "H_in"),             # horizontal pass: rows of a tile (it runs over the INPUT rows)
    "EX4D_RESIZE_V_BYTES": (256, "3 W_out"),       # vertical pass: flat bytes of a tile row, 3 W_out bytes per image row
    "EX4D_RESIZE_V_ROWS": (4, "H_out"),            # vertical pass: output rows of a tile
}
FILTERS = ("bilinear", "box", "bicubic")

# (H_in, W_in, H_out, W_out): the named cases
NAMED = [
    (14, 22, 7, 11),          # exact factor 2
    (15, 23, 7, 11),          # odd input
    (253, 338, 126, 169),     # the dataset's shape over 8
    (33, 65, 16, 32),
    (9, 9, 9, 4),             # horizontal only
    (9, 9, 4, 9),             # vertical only
    (17, 5, 17, 5),           # a copy
    (8, 8, 16, 16),           # up-scaling: ksize 3, taps clipped at both borders
    (7, 13, 10, 19),
    (40, 64, 13, 21),         # non-integer ratio
    (1, 37, 1, 5),
    (37, 1, 5, 1),
    (100, 100, 1, 1),         # 201 taps
    (3, 300, 2, 7),
]


def _tiling_cases():
    """For every tiling constant T: T - 1, T, T + 1 on the axis it tiles, both passes running (the other sizes small, none equal)."""
    out = []
    for T in (TILING["EX4D_RESIZE_H_PIXELS"][0],):
        out += [(6, 2 * w + 1, 3, w) for w in (T - 1, T, T + 1)]
    for T in (TILING["EX4D_RESIZE_H_ROWS"][0],):
        out += [(h, 11, 2, 5) for h in (T - 1, T, T + 1)]
    for T in (TILING["EX4D_RESIZE_V_BYTES"][0],):
        # rows of 3 W_out bytes: 252, 255, 258 straddle T; and T - 1, T, T + 1 pixels (several tiles, the last one part full)
        out += [(5, w + 7, 3, w) for w in (T // 3 - 1, T // 3, T // 3 + 1, T - 1, T, T + 1)]
    for T in (TILING["EX4D_RESIZE_V_ROWS"][0],):
        out += [(2 * h + 1, 9, h, 4) for h in (T - 1, T, T + 1)]
    return out


TILING_CASES = _tiling_cases()
CASES = NAMED + TILING_CASES


def case_id(c):
    return "%dx%d-%dx%d" % c


def random_bytes(H, W, seed=7):
    return np.random.default_rng([seed, H, W]).integers(0, 256, (H, W, 3), dtype=np.uint8)


def saturating(H, W):
    """0 / 255 only: a checkerboard of 3-pixel cells in one channel, columns and rows of alternating runs in the others, so that a
    negative-lobed filter overshoots both ways."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    a = np.empty((H, W, 3), np.uint8)
    a[..., 0] = (((yy // 3) + (xx // 3)) % 2) * 255
    a[..., 1] = ((xx // 2) % 2) * 255
    a[..., 2] = ((yy // 5) % 2) * 255
    return a


CONTENT = {"random": random_bytes, "saturating": saturating}
