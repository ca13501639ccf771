"""RESCAL's workspaces start finite (GPU).  Its kernels multiply the WE / EW
rows and partial scores of an absent negative by a zero coefficient, which
discards a finite stale value and not a NaN; device memory freed by other work
(index buffers holding -1 are NaN bit patterns) may be handed to the next
workspace, so the runners and Model._workspace zero theirs at allocation."""
import numpy as np
import pytest
import torch

import test_gpu_pairloop as TP

pytestmark = pytest.mark.gpu


def test_model_workspace_is_zero_filled():
    m = TP.make_model("rescal", (20, 20, 3), 8)
    poison = torch.full((1 << 20,), float("nan"), device=m.device)
    del poison   # back to the caching allocator: the next request may reuse it
    ws = m._workspace(1 << 20)
    assert ws.numel() >= 1 << 20 and int(ws.count_nonzero().item()) == 0


@pytest.mark.parametrize("loop", ["pairs", "triples"])
def test_typed_rescal_epoch_is_finite_after_nan_memory_was_freed(loop):
    """Typed draws leave absent negatives; the memory freed just before the
    runner is created is all NaN."""
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import DeviceKG, LogisticLoopRunner, PairLoopRunner
    n_ent, n_rel, d = 60, 5, 16
    xs = TP.make_kg(n_ent, n_rel, 299, seed=3)
    m = TP.make_model("rescal", (n_ent, n_ent, n_rel), d)
    m.add_hyperparam("margin", 0.5)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    kg = DeviceKG(xs, m.device)
    torch.cuda.synchronize()
    poison = torch.full((64 << 20,), float("nan"), device=m.device)
    torch.cuda.synchronize()
    del poison
    torch.cuda.empty_cache()   # freed to the driver, where the runner allocates
    cls = PairLoopRunner if loop == "pairs" else LogisticLoopRunner
    r = cls(m, upd, kg, 3, seed=13, ntries=2, sampler=L.SKGE_SAMPLER_TYPED)
    with torch.cuda.stream(r.stream):
        r.run(2)
    r.synchronize()
    for p in m.params.values():
        assert bool(torch.isfinite(p.data).all()), p.name
    assert np.asarray(m.E.updateCounts).sum() > 0
