"""CPU tests of the motion regularisers on several ranks (gloo, the pattern of tests/test_cpu_dist.py): dist.ShardedRAdam.step(reg=...)
adds each term once per step, last, to the reduced gradient -- by the owner of every element -- and every rank ends with the bits of
the replicated update.  The HIP launches are replaced by numpy oracles through the optimizer's hooks (tests/dist_reg_worker.py: test
infrastructure standing in for the kernels; the sharding, the collectives and the order of the additions under test are the product's)."""
import os
import subprocess
import sys

import pytest

from tests import helpers as h

WORKER = os.path.join(h.ROOT, "tests", "dist_reg_worker.py")


def _ranks(world, case, port_base):
    port = port_base + (os.getpid() % 2000)
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, WORKER, h.ROOT, "cpu", case], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=300)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"OK {r}" in o, o


@pytest.mark.parametrize("case", ["dense", "sliced"])
@pytest.mark.parametrize("world", [2, 4])
def test_sharded_radam_with_regularizers_equals_the_replicated_update(world, case):
    """Dense keyframes (element shards that cut rows and keyframes) and sliced keyframes (windows of 4 and 2, whole-row shards): three
    steps, parameters and gathered moments bit-equal to the oracle's update of (reduced gradient + tests/reg_ref.py gradient)."""
    _ranks(world, case, 36100 + 10 * world + (3 if case == "sliced" else 0))


def test_sharded_radam_with_regularizers_off_is_todays_step():
    """reg=None and all-zero weights: the bits of an optimizer built without the new arguments, and no regularised launch."""
    _ranks(2, "off", 38200)


def test_regularizer_weights_views_scales_the_weights_and_keeps_the_gates():
    from ex4dgs_amd.regularizers import regularizer_weights
    opt = dict(progressive_growing_steps=100, make_dynamic_interval=50, extract_every=3, static_reg=1e-4, motion_reg=2e-4, rot_reg=3e-3)
    for iteration in (0, 150, 151, 350, 351, 5000):
        for nd in (0, 7):
            old = regularizer_weights(opt, iteration, nd)
            assert regularizer_weights(opt, iteration, nd, views=1) == old
            six = regularizer_weights(opt, iteration, nd, views=6)
            assert six == tuple(6 * x for x in old)
            assert [x != 0 for x in six] == [x != 0 for x in old]
    assert regularizer_weights(opt, 5000, 7) == (1e-4, 2e-4, 3e-3)
    assert regularizer_weights(opt, 5000, 0, views=6) == (6 * 1e-4, 0.0, 0.0) and regularizer_weights(opt, 151, 7, views=6) == (6 * 1e-4, 0.0, 0.0)
    assert regularizer_weights(opt, 150, 7, views=6) == (0.0, 0.0, 0.0)
    # a term that is off by its own weight stays off
    assert regularizer_weights(dict(opt, rot_reg=0.0), 5000, 7, views=6)[2] == 0.0
