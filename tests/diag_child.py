"""Child process of tests/test_gpu_diag.py: one deterministic pair-loop run.

    python diag_child.py <DistMult|ComplEx> <d> <out.npz>

SKGE_DIAG_PAIRS is read when the runner is created, so each form (k_diag_pos,
the explicit pairs) runs in a process of its own; the parent compares the
tables bit for bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "scikit-kge_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(cls, d, out):
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import DeviceKG, PairLoopRunner
    import test_gpu_diag as TD
    S.set_deterministic(True)
    np.random.seed(11)
    m = getattr(S, cls)((TD.N, TD.N, TD.M), d, rparam=0.01)
    m.add_hyperparam("margin", TD.MARGIN)
    upd = {pid: S.AdaGrad(p, 0.1) for pid, p in m.params.items()}
    assert m.accumulator("E").mode == L.SKGE_ACC_FX64
    r = PairLoopRunner(m, upd, DeviceKG(TD.loop_kg(), m.device), 3, seed=5)
    with torch.cuda.stream(r.stream):
        r.run(2)
    r.synchronize()
    np.savez(out, nviol=int(r.nviol_total.item()), E=m.E.data.cpu().numpy(),
             R=m.R.data.cpu().numpy(), nlaunch=L.lib().skge_pair_runner_nlaunches(r.handle))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3])
