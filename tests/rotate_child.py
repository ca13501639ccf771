"""Child process of tests/test_gpu_rotate.py: one pair-loop run of RotatE.

    python rotate_child.py <d> <opt> <deterministic 0|1> <kg loop|dense> <out.npz>

SKGE_ROT_PAIRS is read when the runner is created, so each form (k_rot_pos, the
explicit pairs) runs in a process of its own.  The child writes the tables
before and after one epoch of 3 batches, the AdaGrad state and the device's own
records; the parent replays them (tests/rotate_ref.py) or compares the two
forms bit for bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "scikit-kge_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED = 5
NB = 3
LR = 0.1


def loop_kg(N, M, T):
    """T distinct triples with a hub subject, some s == o and one frequent relation."""
    import numpy as np
    rs = np.random.RandomState(17)
    seen, out = set(), []
    while len(out) < T:
        s, o, p = int(rs.randint(N)), int(rs.randint(N)), int(rs.randint(M))
        k = len(out)
        if k % 7 == 0:
            s = 3
        elif k % 11 == 0:
            o = s
        if k % 3 == 0:
            p = 1
        if (s, o, p) not in seen:
            seen.add((s, o, p))
            out.append((s, o, p))
    return np.array(out, dtype=np.int32)


def dense_kg():
    """8 entities, 1 relation, every (s, o) but the last known: most corruptions
    cannot be drawn, so the records hold neg = -1."""
    import numpy as np
    out = [(s, o, 0) for s in range(8) for o in range(8)][:-2]
    return np.array(out, dtype=np.int32)


def main(d, opt, det, kgname, out):
    import numpy as np
    import torch
    import skge_amd as S
    from skge_amd import _lib as L
    from skge_amd.device import DeviceKG, PairLoopRunner, epoch_records
    import rotate_ref as RR
    S.set_deterministic(bool(det))
    if kgname == "dense":
        N, M, trip = 8, 1, dense_kg()
    else:
        N, M, trip = RR.N, RR.M, loop_kg(RR.N, RR.M, 3 * 48)
    np.random.seed(11)
    m = S.RotatE((N, N, M), d)
    m.add_hyperparam("margin", 0.5)
    U = S.AdaGrad if opt == "adagrad" else S.SGD
    upd = {pid: U(p, LR) for pid, p in m.params.items()}
    if det:
        assert m.accumulator("E").mode == L.SKGE_ACC_FX64
    kg = DeviceKG(trip, m.device)
    E0, R0 = m.E.data.cpu().numpy(), m.R.data.cpu().numpy()
    r = PairLoopRunner(m, upd, kg, NB, seed=SEED)
    rec, n1 = epoch_records(kg, N, SEED, 0)
    with torch.cuda.stream(r.stream):
        r.run(1)
    r.synchronize()
    p2 = {pid: (upd[pid].p2.cpu().numpy() if opt == "adagrad" else np.zeros(1)) for pid in upd}
    np.savez(out, nviol=int(r.nviol_total.item()), E0=E0, R0=R0, E=m.E.data.cpu().numpy(),
             R=m.R.data.cpu().numpy(), p2E=p2["E"], p2R=p2["R"], rec=rec.cpu().numpy(),
             n1=n1.cpu().numpy(), T=len(trip), N=N, M=M,
             cnt=sum(int(a.cnt.abs().sum().item()) for a in m._acc.values()))


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2], int(sys.argv[3]), sys.argv[4], sys.argv[5])
