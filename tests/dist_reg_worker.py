"""Worker of tests/test_cpu_dist_regularizers.py and tests/test_gpu_dist_regularizers.py: dist.ShardedRAdam.step(reg=...) over gloo.

    python dist_reg_worker.py <repository root> <cpu | cuda> <dense | sliced | off>

Three tensors whose element shards (small_bytes=256, align 4) cut rows and keyframes: _xyz_disp [37,3], _xyz_motion [21,5,3],
_rotation_motion [21,5,4].  Three steps with seeded per-rank gradients and the three terms on; every rank's parameters and gathered
moments must be, bit for bit, the replicated update (oracle/optim_oracle.py) of
    reduced gradient + regulariser gradient (tests/reg_ref.py in float32, at the parameters before the step).
The reduced gradient of a dense tensor is an all-reduce of the same inputs (the collective's own summation order is not under test);
keyframe windows are added in rank order.  On "cpu" the four launches are replaced by numpy oracles through the optimizer's hooks; on
"cuda" the hooks keep their defaults, the HIP launches.  "off": reg=None and all-zero weights are the calls of a step without the
argument (hooks that raise stand where the regularised launches would be)."""
import os
import sys

ROOT, DEVICE, CASE = sys.argv[1:4]
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.distributed as dist

from ex4dgs_amd import dist as xd
from oracle import optim_oracle
from tests import reg_ref

if DEVICE == "cuda":
    os.environ["LOCAL_RANK"] = "0"                   # the ranks share the box's one GPU
rank, world, _ = xd.init_from_env(backend="gloo")
if DEVICE == "cuda":
    from ex4dgs_amd import _C
    torch.cuda.set_device(0); _C.load()
DEV = torch.device("cuda", 0) if DEVICE == "cuda" else torch.device("cpu")

STATIC, MOTION, ROT = 3, 1, 2
SHAPES = [(37, 3), (21, 5, 3), (21, 5, 4)]
KINDS = [STATIC, MOTION, ROT]
LRS = [1e-2, 2e-2, 5e-3]
WEIGHTS = [0.05, 0.08, 0.11]
COUNTS = {1: 4, 2: 2}                                # keyframe windows of the sliced case
STEPS = 3
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def initial():
    g = torch.Generator().manual_seed(3)
    d = 0.02 * torch.randn(37, 3, generator=g)
    m = torch.randn(21, 1, 3, generator=g) + torch.cumsum(0.05 * torch.randn(21, 5, 3, generator=g), 1)
    r = torch.nn.functional.normalize(torch.randn(21, 1, 4, generator=g) + torch.cumsum(0.1 * torch.randn(21, 5, 4, generator=g), 1), dim=-1)
    d[3] = 0                                         # a zero displacement; rows 17 and 18 are where the shards of two ranks cut
    d[17] = 0
    m[5] = m[5, :1]                                  # coincident keyframes
    m[10, 3] = m[10, 0]
    r[2, 1] = 0                                      # a zero keyframe, one below the clamp
    r[10, 4] = r[10, 4] * 1e-8
    return [d.contiguous(), m.contiguous(), r.contiguous()]


def frame(r, step):
    """(dense gradients, {i: (window, first keyframe)}) of rank r at this step."""
    g = torch.Generator().manual_seed(1000 * step + r)
    # multiples of 2^-19 below 2^-7: the sum over four ranks is exact in every order -- a shard's tail travels in the exchange's flat
    # message, where the ring adds the ranks in another order than it does in a whole-tensor all-reduce
    dense = [torch.randint(-4096, 4096, s, generator=g).float() * 2.0 ** -19 for s in SHAPES]
    wins = {}
    for i, count in COUNTS.items():
        first = (step + r + i) % (5 - count + 1) if step != 2 else 0        # step 2: all windows coincide
        wins[i] = (torch.randn(SHAPES[i][0], count, SHAPES[i][2], generator=g) * 1e-3, first)
    return dense, wins


def reg_gradient(kind, p, weight, rows_total):
    """reg_ref's float32 gradient of the rows p (whole rows of a tensor of rows_total rows: the mean's count is the full one)."""
    K = 1 if kind == STATIC else p.shape[1]
    count = rows_total * (1 if kind == STATIC else K - 1)
    coef = np.float32(weight / count) if count else np.float32(0)
    return {STATIC: reg_ref.grad_static, MOTION: reg_ref.grad_motion, ROT: reg_ref.grad_rot}[kind](p, coef, np.float32)


# ---- the numpy oracles that stand for the four launches on the CPU
def oracle_step(items, betas, eps, device):
    for p, g, m, v, n, lr, step, sanitize in items:
        assert not sanitize
        optim_oracle.radam_step(p.numpy(), g.numpy().copy(), m.numpy(), v.numpy(), step, lr, betas[0], betas[1], eps)


def _window_sum(rows, K, C, wins):
    g = np.zeros((rows, K, C), np.float32)
    assert len(wins) == world
    for first, count, t in wins:                     # rank order
        assert tuple(t.shape) == (rows, count, C)
        g[:, first:first + count, :] += t.numpy()
    return g


def oracle_sliced(items, betas, eps, device):
    for p, m, v, rows, K, C, lr, step, wins, first_dev in items:
        optim_oracle.radam_step(p.numpy(), _window_sum(rows, K, C, wins).reshape(-1), m.numpy(), v.numpy(), step, lr, betas[0], betas[1], eps)


def oracle_sliced_reg(items, betas, eps, device):
    for p, m, v, rows, K, C, lr, step, wins, first_dev, kind, weight, reg_rows in items:
        g = _window_sum(rows, K, C, wins)
        if kind:
            assert (kind, C) in ((MOTION, 3), (ROT, 4))
            g += reg_gradient(kind, p.numpy().reshape(rows, K, C), weight, reg_rows)       # the term last
        optim_oracle.radam_step(p.numpy(), g.reshape(-1), m.numpy(), v.numpy(), step, lr, betas[0], betas[1], eps)


def oracle_range(kind, param, lo, hi, grad, weight):
    assert grad.numel() == hi - lo and 0 <= lo < hi <= param.numel()
    g = grad.numpy()
    g += reg_gradient(kind, param.numpy(), weight, param.shape[0]).reshape(-1)[lo:hi]


def refuse(*a, **k):
    raise AssertionError("a regularised launch in a step without regularisers")


def hooks(reg_hooks=True):
    if DEVICE == "cuda":
        return {}
    out = dict(step_fn=oracle_step, sliced_step_fn=oracle_sliced)
    if reg_hooks:
        out.update(sliced_reg_step_fn=oracle_sliced_reg, reg_range_fn=oracle_range)
    return out


def reduced(i, step):
    """Sum over the ranks of tensor i's dense gradient: an all-reduce of the same inputs (a collective: every rank calls it)."""
    g = frame(rank, step)[0][i].clone()
    dist.all_reduce(g)
    return g.numpy()


def run(sliced):
    init = initial()
    params = [x.clone().to(DEV) for x in init]
    opt = xd.ShardedRAdam(params, LRS, small_bytes=256, sliced=(COUNTS if sliced else None), **hooks())
    assert opt.small == [False, False, False]
    if not sliced:                                   # the element shards cut a row of every tensor and a keyframe of the keyframe tensors
        edges = [[xd.shard_range(init[i].numel(), r, world)[0] for r in range(1, world)] for i in range(3)]
        assert opt.owned[1] == xd.shard_range(315, rank, world)[:2]
        assert all(any(e % (5 * SHAPES[i][2]) for e in edges[i]) for i in (1, 2)), edges             # inside a row of each keyframe tensor
        assert any(e % SHAPES[i][-1] for i in range(3) for e in edges[i]), edges                    # between the components of a row / keyframe
        assert any(e % (5 * 3) and not e % 3 for e in edges[1]), edges                              # between two keyframes of a row
    ref = [x.clone().numpy() for x in init]
    m = [np.zeros_like(x) for x in ref]; v = [np.zeros_like(x) for x in ref]
    reg = {i: (KINDS[i], WEIGHTS[i], SHAPES[i][0]) for i in range(3)}
    for step in range(1, STEPS + 1):
        dense, wins = frame(rank, step)
        sums = [None if (sliced and i in COUNTS) else reduced(i, step) for i in range(3)]     # (before the exchange reduces `dense` in place)
        opt.launch_exchange([g.to(DEV) for g in dense], windows=({i: (w.to(DEV), f) for i, (w, f) in wins.items()} if sliced else None))
        opt.step(reg=reg)
        frames = [frame(r, step) for r in range(world)]
        for i in range(3):
            if sums[i] is None:
                g = np.zeros(SHAPES[i], np.float32)
                for r in range(world):
                    w, first = frames[r][1][i]
                    g[:, first:first + w.shape[1]] += w.numpy()
            else:
                g = sums[i]
            g = g + reg_gradient(KINDS[i], ref[i], WEIGHTS[i], SHAPES[i][0])
            optim_oracle.radam_step(ref[i].reshape(-1), g.reshape(-1), m[i].reshape(-1), v[i].reshape(-1), step, LRS[i])
        if DEVICE == "cuda":
            torch.cuda.synchronize()
        moments = opt.full_moments()
        for i in range(3):
            assert np.array_equal(bits(params[i].cpu().numpy()), bits(ref[i])), ("param", sliced, i, step, rank)
            assert np.array_equal(bits(moments[i][0].cpu().numpy()), bits(m[i])), ("exp_avg", sliced, i, step, rank)
            assert np.array_equal(bits(moments[i][1].cpu().numpy()), bits(v[i])), ("exp_avg_sq", sliced, i, step, rank)
    # the terms were live: without them the parameters end elsewhere
    plain = [x.clone().to(DEV) for x in init]
    opt0 = xd.ShardedRAdam(plain, LRS, small_bytes=256, sliced=(COUNTS if sliced else None), **hooks())
    dense, wins = frame(rank, 1)
    opt0.launch_exchange([g.to(DEV) for g in dense], windows=({i: (w.to(DEV), f) for i, (w, f) in wins.items()} if sliced else None))
    opt0.step()
    first = [x.clone().to(DEV) for x in init]
    opt1 = xd.ShardedRAdam(first, LRS, small_bytes=256, sliced=(COUNTS if sliced else None), **hooks())
    dense, wins = frame(rank, 1)
    opt1.launch_exchange([g.to(DEV) for g in dense], windows=({i: (w.to(DEV), f) for i, (w, f) in wins.items()} if sliced else None))
    opt1.step(reg=reg)
    assert all(not torch.equal(a, b) for a, b in zip(plain, first))


def off(sliced):
    """reg=None and all-zero weights against an optimizer built without the new arguments, calling step() as before."""
    init = initial()
    kw = dict(small_bytes=256, sliced=(COUNTS if sliced else None))
    old = dict(step_fn=oracle_step, sliced_step_fn=oracle_sliced) if DEVICE == "cpu" else {}
    new = dict(old, sliced_reg_step_fn=refuse, reg_range_fn=refuse)
    runs = []
    for hook, reg in ((old, "absent"), (new, None), (new, {i: (KINDS[i], 0.0, SHAPES[i][0]) for i in range(3)})):
        params = [x.clone().to(DEV) for x in init]
        opt = xd.ShardedRAdam(params, LRS, **kw, **hook)
        for step in range(1, STEPS + 1):
            dense, wins = frame(rank, step)
            opt.launch_exchange([g.to(DEV) for g in dense], windows=({i: (w.to(DEV), f) for i, (w, f) in wins.items()} if sliced else None))
            if reg == "absent":
                opt.step()
            else:
                opt.step(reg=reg)
        runs.append((params, opt.full_moments()))
    for params, moments in runs[1:]:
        for i in range(3):
            assert np.array_equal(bits(params[i].cpu().numpy()), bits(runs[0][0][i].cpu().numpy())), (sliced, i)
            for a, b in zip(moments[i], runs[0][1][i]):
                assert np.array_equal(bits(a.cpu().numpy()), bits(b.cpu().numpy())), (sliced, i)
    assert not torch.equal(runs[0][0][1].cpu(), init[1])


if CASE == "off":
    off(False); off(True)
else:
    run(CASE == "sliced")
if DEVICE == "cuda":
    torch.cuda.synchronize()
dist.barrier(); dist.destroy_process_group()
print("OK", rank)
