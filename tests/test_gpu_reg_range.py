"""GPU tests of ex4d_reg_backward_range (include/ex4d_regularizers.h; regularizers.backward_range_raw): one term's gradient over a flat
element range of its tensor -- what a rank of the sharded optimizer adds to the elements it owns -- against the slice of the dense
ex4d_reg_backward, bit for bit.  The dense call is pinned to the reference's lines by tests/test_gpu_regularizers.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

STATIC, MOTION, ROT = 3, 1, 2
WIDTH = {STATIC: 3, MOTION: 3, ROT: 4}
WEIGHT = 0.37
GUARD = 5                          # guard elements on either side of the shard buffer (an odd count: the buffer is not 16-byte aligned)
bits = lambda t: t.contiguous().view(torch.int32)


def tensor(kind, rows, K, seed):
    """Seeded parameters with the edge rows of the regularisers: a zero displacement, coincident keyframes, rotation keyframes that are
    zero and below the 1e-6 clamp."""
    g = torch.Generator().manual_seed(seed)
    if kind == STATIC:
        p = 0.02 * torch.randn(rows, 3, generator=g)
        if rows > 1:
            p[rows // 2] = 0
    elif kind == MOTION:
        p = torch.randn(rows, 1, 3, generator=g) + torch.cumsum(0.05 * torch.randn(rows, K, 3, generator=g), 1)
        if rows > 1:
            p[rows // 2] = p[rows // 2, :1]                     # every keyframe equals keyframe 0
        if K > 2:
            p[0, K - 1] = p[0, 0]                               # one coincident keyframe
    else:
        p = torch.nn.functional.normalize(torch.randn(rows, 1, 4, generator=g) + torch.cumsum(0.1 * torch.randn(rows, K, 4, generator=g), 1), dim=-1)
        p = p * (1 + 0.05 * torch.randn(rows, K, 1, generator=g))
        if K > 1:
            p[0, 1] = p[0, 1] / p[0, 1].norm() * 1e-8           # below the clamp
        if rows > 1:
            p[rows - 1, 0] = 0
    return p.contiguous().cuda()


def dense(kind, p, weight, out, accumulate):
    """ex4d_reg_backward of this term alone over the whole tensor."""
    from ex4dgs_amd import regularizers as reg
    slot = {STATIC: 0, MOTION: 1, ROT: 2}[kind]
    params, grads, w = [None] * 3, [None] * 3, [0.0] * 3
    params[slot], grads[slot], w[slot] = p, out, weight
    reg.backward_raw(*params, w, grads, accumulate=accumulate)
    return out


def ranges(kind, rows, K):
    from ex4dgs_amd.dist import shard_range
    C = WIDTH[kind]
    per = C * (1 if kind == STATIC else K)
    n = rows * per
    out = [(0, n), (n // 2, n // 2 + 1), (n - 1, n), (n // 3, n // 3), (0, 0), (n, n)]
    out += [shard_range(n, r, W, align=4)[:2] for W in (2, 3, 8) for r in range(W)]
    out.append(((rows // 2) * per, (rows // 2) * per + 1))                   # the first component of a keyframe 0: the sum over the row
    if rows > 1:
        # from the second component of a keyframe (the last of row 0) to the first component of another row's keyframe 0
        out.append((per - C + 1, (rows - 1) * per + 1))
        out.append((1, per + 1))
    if per > C:
        out.append((C + 2, per - 1))                                        # inside one row, cut inside its keyframes at both ends
    return out


def guarded(n, fill=None):
    buf = torch.full((n + 2 * GUARD,), -1, dtype=torch.int32, device="cuda")       # 0xFFFFFFFF
    view = buf.view(torch.float32)[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def guards_intact(buf, n):
    return bool((buf[:GUARD] == -1).all()) and bool((buf[GUARD + n:] == -1).all())


def shapes(kind):
    return [(rows, K) for rows in (1, 5, 257) for K in ((1,) if kind == STATIC else (1, 2, 3, 35))]


@pytest.mark.parametrize("kind", [STATIC, MOTION, ROT], ids=["static", "motion", "rot"])
def test_range_gradient_equals_the_slice_of_the_dense_gradient(hip_lib, kind):
    from ex4dgs_amd import regularizers as reg
    live = 0
    for rows, K in shapes(kind):
        p = tensor(kind, rows, K, 100 * rows + K)
        base = 1e-3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(rows + K)).cuda()
        want_write = dense(kind, p, WEIGHT, torch.full_like(p, float("nan")), False).view(-1)
        want_add = dense(kind, p, WEIGHT, base.clone(), True).view(-1)
        want_zero = dense(kind, p, 0.0, torch.full_like(p, float("nan")), False).view(-1)
        assert float(want_zero.abs().max()) == 0.0
        live += int(want_write.count_nonzero())
        flat = base.view(-1)
        for lo, hi in ranges(kind, rows, K):
            n, tag = hi - lo, (kind, rows, K, lo, hi)
            buf, g = guarded(n)
            reg.backward_range_raw(kind, p, lo, hi, g, WEIGHT, accumulate=False)
            assert torch.equal(bits(g), bits(want_write[lo:hi])) and guards_intact(buf, n), ("write", tag)
            buf, g = guarded(n, flat[lo:hi])
            reg.backward_range_raw(kind, p, lo, hi, g, WEIGHT)                                   # accumulate is the default
            assert torch.equal(bits(g), bits(want_add[lo:hi])) and guards_intact(buf, n), ("accumulate", tag)
            # weight 0: zeros in write mode, the buffer untouched in accumulate mode
            buf, g = guarded(n)
            reg.backward_range_raw(kind, p, lo, hi, g, 0.0, accumulate=False)
            assert torch.equal(bits(g), bits(want_zero[lo:hi])) and guards_intact(buf, n), ("zero write", tag)
            buf, g = guarded(n, flat[lo:hi])
            reg.backward_range_raw(kind, p, lo, hi, g, 0.0, accumulate=True)
            assert torch.equal(bits(g), bits(flat[lo:hi])) and guards_intact(buf, n), ("zero accumulate", tag)
    assert live > 0


def test_range_refusals_and_their_texts(hip_lib):
    from ex4dgs_amd import _abi
    from ex4dgs_amd import regularizers as reg
    p = tensor(MOTION, 5, 3, 1)                                  # 45 elements
    buf, g = guarded(8)
    lib = _abi.load()
    for lo, hi in ((-1, 7), (40, 48), (0, 46)):
        with pytest.raises(RuntimeError, match=r"element range \[-?\d+, \d+\) is not inside the tensor's \[0, 45\)"):
            reg.backward_range_raw(MOTION, p, lo, hi, g if hi - lo == 8 else torch.empty(hi - lo, device="cuda"), WEIGHT)
        assert b"element range" in lib.ex4d_reg_last_error()
    with pytest.raises(RuntimeError, match="element range"):     # lo > hi
        reg.backward_range_raw(MOTION, p, 9, 3, torch.empty(0, device="cuda"), WEIGHT)
    with _abi.stream(p.device) as stream:
        for kind in (0, 4, -1):
            with pytest.raises(RuntimeError, match=f"unknown kind {kind}"):
                _abi.call("ex4d_reg_backward_range", kind, p.data_ptr(), 5, 3, 0, 8, g.data_ptr(), WEIGHT, 1, stream)
        with pytest.raises(RuntimeError, match="K < 1"):
            _abi.call("ex4d_reg_backward_range", ROT, p.data_ptr(), 5, 0, 0, 8, g.data_ptr(), WEIGHT, 1, stream)
        with pytest.raises(RuntimeError, match="null parameter or gradient"):
            _abi.call("ex4d_reg_backward_range", MOTION, p.data_ptr(), 5, 3, 0, 8, None, WEIGHT, 1, stream)
        # an empty range is fine wherever it lies, without a launch: null pointers are never read
        _abi.call("ex4d_reg_backward_range", MOTION, None, 5, 3, 45, 45, None, WEIGHT, 0, stream)
        assert lib.ex4d_reg_last_error() == b""
    with pytest.raises(RuntimeError, match="unknown kind"):
        reg.backward_range_raw(0, p, 0, 8, g, WEIGHT)
    with pytest.raises(RuntimeError, match="hi - lo elements"):
        reg.backward_range_raw(MOTION, p, 0, 9, g, WEIGHT)
    with pytest.raises(RuntimeError, match="hi - lo elements"):
        reg.backward_range_raw(MOTION, p, 0, 8, g.double(), WEIGHT)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        reg.backward_range_raw(MOTION, p.cpu(), 0, 8, g.cpu(), WEIGHT)
    with pytest.raises(RuntimeError, match=r"\[Nd, K, 4\]"):
        reg.backward_range_raw(ROT, p, 0, 8, g, WEIGHT)
    torch.cuda.synchronize()
    assert guards_intact(buf, 8) and bool((buf[GUARD:GUARD + 8] == -1).all())       # no refused call wrote anything


def test_range_call_replays_from_a_graph(hip_lib):
    from ex4dgs_amd import regularizers as reg
    from ex4dgs_amd.dist import shard_range
    for kind in (STATIC, MOTION, ROT):
        p = tensor(kind, 257, 35, 9)
        lo, hi = shard_range(p.numel(), 1, 3)[:2]
        base = torch.randn(hi - lo, generator=torch.Generator().manual_seed(2)).cuda() * 1e-3
        eager, graphed = base.clone(), base.clone()
        reg.backward_range_raw(kind, p, lo, hi, eager, WEIGHT)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            reg.backward_range_raw(kind, p, lo, hi, graphed, WEIGHT)      # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            reg.backward_range_raw(kind, p, lo, hi, graphed, WEIGHT)
        graphed.copy_(base)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(graphed), bits(eager)) and not torch.equal(eager, base), kind
