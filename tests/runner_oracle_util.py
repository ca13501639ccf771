"""Replay of a device epoch through the fp64 oracle, shared by the runner
oracle tests (test_gpu_runner_oracle.py, test_gpu_rescal_rows.py).

The oracle replays the pairs the device drew (skge_epoch_sample, the same
keyed draws the runners make) in the order
PairwiseStochasticTrainer._process_batch builds them (skge/base.py:1394-1427),
from the device state snapshotted before them."""
import numpy as np

import parity_util
from oracle import skge_oracle as O


def pairs(rec, n1, start, count):
    pos, neg = [], []
    for j in range(start, start + count):
        s, o, p, a = (int(x) for x in rec[j])
        b = int(n1[j])
        if a >= 0:
            pos.append((s, o, p))
            neg.append((a, o, p))
        if b >= 0:
            pos.append((s, o, p))
            neg.append((s, b, p))
    return (np.array(pos, dtype=np.int64).reshape(-1, 3),
            np.array(neg, dtype=np.int64).reshape(-1, 3))


def snapshot(m, upd):
    params = {pid: p.data.detach().cpu().numpy().astype(np.float64) for pid, p in m.params.items()}
    state = {pid: upd[pid].p2.detach().cpu().numpy().astype(np.float64)
             for pid in m.params if getattr(upd[pid], "p2", None) is not None}
    return params, state


def _rows_of(grads, rows):
    """(g, idx) restricted to `rows` and re-indexed into them."""
    if grads is None:
        return None
    g, idx = grads
    idx = np.asarray(idx, dtype=np.int64)
    pos = {int(r): i for i, r in enumerate(rows)}
    keep = [i for i, r in enumerate(idx) if int(r) in pos]
    if not keep:
        return None
    return (np.asarray(g)[keep], np.array([pos[int(idx[i])] for i in keep], dtype=np.int64))


def epoch_vs_oracle(kind, m, upd, runner, kg, seed, epoch, nb, opt, what, n_ent, sizes=None,
                    all_found=True, ntries=100, lr=0.1, batch_hook=None, groups=None, **kw):
    """Run epoch `epoch` (0-based; the runner's key is at it) on the device and
    replay its batches through the oracle from the device state before it.

    sizes: the batch sizes the caller expects (asserted); all_found: every
    negative of the epoch was found (asserted).  batch_hook(rec, n1, start,
    count, before, grads) sees every batch with the oracle's parameters before
    it and its gradients (None: no violation).  groups: {pid: callable ->
    {name: rows}}, evaluated after the replay: that table is checked group by
    group (and the rows in no group as "other"), each with a headroom record
    named after the group.  Returns the epoch's violations."""
    from skge_amd.device import batch_sizes, epoch_records
    params, state = snapshot(m, upd)
    if opt == "sgd":
        state = {k: np.zeros_like(v) for k, v in params.items()}
    v0 = int(runner.nviol_total.item())
    rec, n1 = epoch_records(kg, n_ent, seed, epoch, ntries=ntries)
    rec, n1 = rec.cpu().numpy(), n1.cpu().numpy()
    runner.run(1)
    runner.synchronize()
    got_v = int(runner.nviol_total.item()) - v0
    want_v, start = 0, 0
    got_sizes = batch_sizes(kg.T, nb)
    if sizes is not None:
        assert got_sizes == list(sizes), (got_sizes, sizes)
    before, grads = {k: v.copy() for k, v in params.items()}, None
    for c in got_sizes:
        pos, neg = pairs(rec, n1, start, c)
        if all_found:
            assert len(pos) == 2 * c          # every negative found
        before = {k: v.copy() for k, v in params.items()}
        grads, nv = None, 0
        if len(pos):
            _, _, nv, grads = O.pairwise_step(kind, params, state, pos, neg, lr, float(m.margin),
                                              opt, **kw)
        if batch_hook is not None:
            batch_hook(rec, n1, start, c, before, grads)
        start += c
        want_v += nv
    assert got_v == want_v, (what, got_v, want_v)
    for pid in m.params:
        sel = {"": None}
        if groups and pid in groups:
            sel = {k: np.asarray(v, dtype=np.int64) for k, v in groups[pid]().items()}
            rest = np.ones(params[pid].shape[0], dtype=bool)
            for v in sel.values():
                rest[v] = False
            sel["other"] = np.nonzero(rest)[0]
        got = m.params[pid].data.detach().cpu().numpy()
        p2 = upd[pid].p2.detach().cpu().numpy() if opt == "adagrad" else None
        for name, rows in sel.items():
            if rows is not None and len(rows) == 0:
                continue
            tag = "%s %s%s" % (what, pid, " [%s rows]" % name if name else "")
            cut = (lambda a: a) if rows is None else (lambda a, rows=rows: a[rows])
            if nb == 1:     # one step from the snapshot: the step-aware bound (parity_util.check_step)
                g = grads[pid] if grads else None
                parity_util.check_step(cut(got), cut(params[pid]), cut(before[pid]),
                                       g if rows is None else _rows_of(g, rows), cut(state[pid]),
                                       lr, tag, post=parity_util.POSTS[kind].get(pid), opt=opt)
            else:
                parity_util.check(cut(got), cut(params[pid]), tag,
                                  lr=lr if opt == "adagrad" else None,
                                  p2=cut(state[pid]) if opt == "adagrad" else None)
            if opt == "adagrad":
                parity_util.check(cut(p2), cut(state[pid]), "%s p2 %s%s"
                                  % (what, pid, " [%s rows]" % name if name else ""))
    return got_v
