"""Host side of the device logistic loop (CPU): the C ABI names in the header
and the ctypes table, and StochasticTrainer's device_loop / seed / ntries
kwargs (stored without a device; PairwiseStochasticTrainer's stay its own)."""
import os
import re
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["skge_triple_runner_create", "skge_triple_runner_run", "skge_triple_runner_nlaunches",
         "skge_triple_runner_destroy"]


class _Update(object):
    def __init__(self, param, learning_rate):
        self.param, self.learning_rate = param, learning_rate


def _model():
    return types.SimpleNamespace(params={"E": object(), "R": object()},
                                 add_hyperparam=lambda *a: None)


def test_runner_names_in_header_and_ctypes_table():
    from skge_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "skge_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["skge_triple_runner_create"][1]) == 14
    assert "#define SKGE_ABI_VERSION 2" in src


def test_stochastic_trainer_stores_device_loop_kwargs():
    from skge_amd.base import PairwiseStochasticTrainer, StochasticTrainer
    t = StochasticTrainer(_model(), param_update=_Update)
    assert (t.device_loop, t.seed, t.ntries, t._runner) == (False, 0, 100, None)
    t = StochasticTrainer(_model(), param_update=_Update, device_loop=True, seed=7, ntries=13)
    assert (t.device_loop, t.seed, t.ntries, t._runner) == (True, 7, 13, None)
    p = PairwiseStochasticTrainer(_model(), param_update=_Update, device_loop=True, seed=3,
                                  ntries=9, file_grad=None, file_embed=None)
    assert (p.device_loop, p.seed, p.ntries, p.device_runner) == (True, 3, 9, "auto")
    p = PairwiseStochasticTrainer(_model(), param_update=_Update, file_grad=None, file_embed=None)
    assert (p.device_loop, p.seed, p.ntries) == (False, 0, 100)
