"""The plan export against the runners built from the same tables (GPU), on
test_gpu_pipe_instances.py's KGs: what skge_pipe_runner_plan answers without
a device is what the constructor builds.  Building a runner also runs the
constructor's own check that its allocations add up to the plan's bytes."""
import pytest

from test_gpu_pipe_instances import _kg, _runner

pytestmark = pytest.mark.gpu

KERNELS = ("k_pipe_batch", "k_pipe_fused", "k_hole_pipe")
HOT_MAX = 256


def _plan(r, d, nb, hole=0):
    from skge_amd import _lib as L
    p = L.SkgePipePlan()
    L.check(L.lib().skge_pipe_runner_plan(r.te, r.tr, d, r.kg.T, nb, 0, hole, p), "plan")
    return p


@pytest.mark.parametrize("kind,d,nb", [("uniform", 64, 3), ("uniform", 200, 3),
                                       ("uniform", 260, 3), ("zipf", 200, 10)])
def test_plan_is_what_the_transe_runner_built(kind, d, nb):
    n_ent, n_rel, trip = _kg(kind)
    m, upd, r = _runner(trip, n_ent, n_rel, d, nb, pipelined=True)
    p = _plan(r, d, nb)
    assert KERNELS[p.kernel] == r.kernel == ("k_pipe_fused" if d == 64 else "k_pipe_batch")
    assert bool(p.e8) == bool(r.ent_i8)
    assert bool(p.w32) == bool(r.rel_w32)
    assert p.nlaunches == r.nlaunches
    assert p.kq == (2 if d == 260 else 1)
    if kind == "zipf":
        assert 0 < r.hot_rows <= HOT_MAX
    else:
        assert r.hot_rows == 0


def test_plan_is_what_the_hole_runner_built():
    import numpy as np
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import DeviceKG, HolePipeRunner
    n_ent, n_rel, trip = _kg("uniform")
    np.random.seed(11)
    m = S.HolE((n_ent, n_ent, n_rel), 200)
    assert HolePipeRunner.eligible(m)
    m.add_hyperparam("margin", 0.2)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    r = HolePipeRunner(m, upd, DeviceKG(trip, m.device), 3, seed=11)
    p = _plan(r, 200, 3, hole=1)
    assert p.kernel == L.lib().skge_pipe_runner_kernel(r.handle) == 2
    assert (p.e8, p.w32, p.fft, p.pair) == (0, 0, 1, 1)
    assert p.nlaunches == r.nlaunches
