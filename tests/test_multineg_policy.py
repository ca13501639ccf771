"""Which (n, modes) the device loops take (skge_amd.device.device_sampler_args,
CPU): for a trainer built with device_negatives=True any n >= 1 over 1 to 8
modes from {0, 1, 2} with n * len(modes) <= 64, for the three sampler classes;
(1, [0, 1]) reported as it always was; without the switch anything else stays
on the per-batch path, as it always has."""
import types

import multineg_ref as MR

N, M, XS = MR.N, MR.M, MR.XS


def _args(samplef, xs=XS, device_negatives=True):
    from skge_amd.device import device_sampler_args
    model = types.SimpleNamespace(E=types.SimpleNamespace(rows=N), sz=(N, N, M))
    trainer = types.SimpleNamespace(samplef=samplef, ntries=100, model=model,
                                    device_negatives=device_negatives)
    return device_sampler_args(trainer, xs, [1] * len(xs))


def test_more_negatives_and_relation_corruption_are_eligible():
    from skge_amd import _lib as L
    from skge_amd.sample import CorruptedSampler, LCWASampler, RandomModeSampler, type_index
    sz = (N, N, M)
    cases = [(RandomModeSampler(3, [0, 1], XS, sz), L.SKGE_SAMPLER_RANDOM, 3, [0, 1], None),
             (LCWASampler(2, [0, 1, 2], XS, sz), L.SKGE_SAMPLER_LCWA, 2, [0, 1, 2], None),
             (CorruptedSampler(1, XS, type_index(XS), modes=[2]), L.SKGE_SAMPLER_TYPED, 1, [2],
              MR.REL_RANGE),
             (RandomModeSampler(8, [1, 0, 0, 2, 2, 1, 0, 1], XS, sz), L.SKGE_SAMPLER_RANDOM, 8,
              [1, 0, 0, 2, 2, 1, 0, 1], None)]
    for smp, kind, n, modes, rel_range in cases:
        smp.ntries = 37
        a = _args(smp.sample)
        ok, ntries, why = a   # unpacks as it always has
        assert ok and ntries == 37 and why == "", (type(smp).__name__, why)
        assert (a.kind, a.n, a.modes, a.rel_range) == (kind, n, modes, rel_range)
        assert a.negatives == (n, modes, rel_range)


def test_one_negative_per_mode_is_reported_as_before():
    from skge_amd.sample import CorruptedSampler, LCWASampler, RandomModeSampler, type_index
    sz = (N, N, M)
    for kind, smp in enumerate((RandomModeSampler(1, [0, 1], XS, sz),
                                CorruptedSampler(1, XS, type_index(XS)),
                                LCWASampler(1, (0, 1), XS, sz))):
        for switch in (True, False):
            a = _args(smp.sample, device_negatives=switch)
            assert tuple(a) == (True, 100, "") and a.kind == kind
            assert (a.n, a.modes, a.rel_range) == (1, [0, 1], None)


def test_without_the_switch_more_negatives_stay_on_the_per_batch_path():
    from skge_amd.sample import CorruptedSampler, LCWASampler, RandomModeSampler, type_index
    sz = (N, N, M)
    for smp, what in ((RandomModeSampler(3, [0, 1], XS, sz), "n=3"),
                      (LCWASampler(2, [0, 1, 2], XS, sz), "modes=[0, 1, 2]"),
                      (CorruptedSampler(1, XS, type_index(XS), modes=[2]), "modes=[2]")):
        a = _args(smp.sample, device_negatives=False)
        assert not a[0] and what in a[2] and "is not (1, [0, 1])" in a[2]
        assert "device_negatives=True" in a[2]      # the reason names the switch
        assert (a.kind, a.n, a.modes) == (0, 1, [0, 1])
        assert _args(smp.sample)[0]                 # and with it they are taken


def test_trainers_take_the_switch():
    """The kwarg is popped by both trainers, off by default (no device needed:
    a model stand-in with no parameters)."""
    from skge_amd.base import PairwiseStochasticTrainer, StochasticTrainer
    model = types.SimpleNamespace(params={}, add_hyperparam=lambda k, v: None)
    assert StochasticTrainer(model).device_negatives is False
    assert StochasticTrainer(model, device_negatives=True).device_negatives is True
    kw = dict(file_grad=None, file_embed=None)
    assert PairwiseStochasticTrainer(model, **kw).device_negatives is False
    assert PairwiseStochasticTrainer(model, device_negatives=True, **kw).device_negatives is True


def test_out_of_scope_negatives_are_ineligible_with_a_reason():
    from skge_amd.sample import CorruptedSampler, LCWASampler, RandomModeSampler, type_index
    sz = (N, N, M)
    cases = [(RandomModeSampler(1, [3], XS, sz), "modes=[3]"),
             (RandomModeSampler(33, [0, 1], XS, sz), "66 negatives"),
             (LCWASampler(1, [], XS, sz), "modes=[]"),
             (CorruptedSampler(1, XS, type_index(XS), modes=[0, -1]), "modes=[0, -1]"),
             (RandomModeSampler(0, [0, 1], XS, sz), "n=0"),
             (RandomModeSampler(1, [0] * 9, XS, sz), "1 to 8 modes"),
             # a mode 2 draws randint(sz[2]): it must be the model's relation count
             (RandomModeSampler(1, [2], XS, (N, N, M + 1)), "sizes")]
    for smp, what in cases:
        a = _args(smp.sample)
        assert not a[0] and what in a[2], (what, a[2])
        assert (a.kind, a.n, a.modes) == (0, 1, [0, 1])


def test_explicit_fused_runner_refuses_more_negatives():
    """make_runner's refusal comes before anything touches the device."""
    import pytest
    from skge_amd.device import make_runner
    for runner in ("epoch", "hole_pipe"):
        with pytest.raises(ValueError, match="pairs"):
            make_runner(None, None, None, 3, runner=runner, negatives=(3, [0, 1], None))
