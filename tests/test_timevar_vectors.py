"""The fitted vector of a ``timevar`` worker without a device: the split into orbit, GP and time-scale parts
(``utils.convert_vectors_timevar``) and its inverse, the ``timevar`` block, the prior on the time scales, the ``timevar:``
block of config.yaml, and -- on the float64 CPU reference -- that three defects of the batch route would be seen by the
value test of tests/test_gpu_timevar_sampling.py."""
import numpy as np
import pytest

from psoap_amd import priors, sample_parallel, utils
from psoap_amd import synthetic as syn

INF = float("inf")
PARS = dict(zip(utils.registered_params["SB2"], syn.ORBIT_BASE["SB2"] + syn.GP_BASE[2]))


def _model_vectors(B, fix=()):
    p0 = utils.convert_dict("SB2", fix, **PARS)
    return p0[None, :] * (1.0 + 0.01 * np.arange(B)[:, None])


@pytest.mark.parametrize("fit,fix", [((True, True), ()), ((False, True), ()), ((True, False), ("gamma", "l_g")), ((False, False), ("q",))])
def test_split_and_join(fit, fix):
    B, defaults = 4, np.array([30.0, INF])
    pm = _model_vectors(B, fix)
    taus = np.array([[5.0 + b, 90.0 - b] for b in range(B)])
    ps = utils.join_vectors_timevar(pm, taus, fit)
    n_tau = sum(fit)
    assert ps.shape == (B, pm.shape[1] + n_tau)
    p_orb, p_gp, got = utils.convert_vectors_timevar(ps, "SB2", fix, fit, defaults, **PARS)
    # the model part is exactly convert_vectors' output
    want_orb, want_gp = utils.convert_vectors(pm, "SB2", fix, **PARS)
    assert np.array_equal(p_orb, want_orb) and np.array_equal(p_gp, want_gp)
    assert got.shape == (B, 2) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
    for k in range(2):
        assert np.array_equal(got[:, k], taus[:, k] if fit[k] else np.full(B, defaults[k]))
    # fitted time scales follow the model's vector in component order
    assert np.array_equal(ps[:, pm.shape[1]:], taus[:, np.array(fit)])


def test_defaults_at_inf_and_three_components():
    reg = utils.registered_params["ST3"]
    pars = dict(zip(reg, syn.ORBIT_BASE["ST3"] + syn.GP_BASE[3]))
    pm = utils.convert_dict("ST3", (), **pars)[None, :]
    ps = utils.join_vectors_timevar(pm, [INF, 12.0, INF], (False, True, False))
    assert ps.shape == (1, len(reg) + 1) and ps[0, -1] == 12.0
    _, _, taus = utils.convert_vectors_timevar(ps, "ST3", (), (False, True, False), (INF, 40.0, INF), **pars)
    assert np.array_equal(taus, [[INF, 12.0, INF]])
    # nothing fitted: the vector is the model's, the time scales the defaults
    _, _, taus = utils.convert_vectors_timevar(pm, "ST3", (), (False,) * 3, (INF, 40.0, INF), **pars)
    assert np.array_equal(taus, [[INF, 40.0, INF]])


def test_wrong_length_is_refused():
    pm = _model_vectors(2)
    with pytest.raises(ValueError, match=r"11 \+ 1"):
        utils.convert_vectors_timevar(pm, "SB2", (), (True, False), (30.0, INF), **PARS)
    with pytest.raises(ValueError, match=r"11 \+ 0"):
        utils.convert_vectors_timevar(np.hstack([pm, pm[:, :1]]), "SB2", (), (False, False), (30.0, INF), **PARS)
    with pytest.raises(ValueError):
        utils.convert_vectors_timevar(pm[0], "SB2", (), (False, False), (30.0, INF), **PARS)


def test_timevar_block_is_checked():
    fit, tau, times = utils.timevar_spec("SB2", {"fit": [True, False], "tau": [30.0, INF]})
    assert fit.tolist() == [True, False] and tau.tolist() == [30.0, INF] and times is None
    fit, tau, _ = utils.timevar_spec("SB1", {})
    assert fit.tolist() == [False] and tau.tolist() == [INF]
    for bad in ({"fit": [True]}, {"tau": [1.0]}, {"fit": [1, 0]}, {"tau": [0.0, 1.0]}, {"tau": [-1.0, 1.0]},
                {"tau": [float("nan"), 1.0]}, {"taus": [1.0, 1.0]}):
        with pytest.raises(ValueError):
            utils.timevar_spec("SB2", bad)


def test_prior_on_the_time_scales_needs_no_device():
    pm = _model_vectors(5)
    ps = utils.join_vectors_timevar(pm, [[3.0, 1.0], [0.0, 1.0], [-2.0, 1.0], [float("nan"), 1.0], [INF, 1.0]], (True, False))
    prior = priors.make_prior_timevar("SB2", (), (True, False), **PARS)
    assert prior(ps).tolist() == [0.0, -INF, -INF, -INF, 0.0]
    # the model part still goes through the model's box
    ps[0, 0] = -1.0          # q < 0
    assert prior(ps)[0] == -INF
    # nothing fitted: the model's prior itself
    assert np.array_equal(priors.make_prior_timevar("SB2", (), (False, False), **PARS)(pm), priors.make_prior("SB2", (), **PARS)(pm))


def test_config_block():
    cfg = {"model": "SB2", "fix_params": [], "jumps": {k: 0.1 for k in PARS}, "opt_jump": "/nonexistent.npy"}
    assert sample_parallel.timevar_block(cfg) is None
    cfg["timevar"] = {"fit": [True, False], "tau": [25.0, INF], "jumps": [2.0, 0.0]}
    tv = sample_parallel.timevar_block(cfg)
    assert tv["fit"].tolist() == [True, False] and tv["tau"].tolist() == [25.0, INF]
    cov = sample_parallel.proposal_covariance(cfg, "SB2", 12, tv)
    assert cov.shape == (12, 12) and cov[-1, -1] == 4.0 and cov[0, 0] == pytest.approx(0.01)
    assert sample_parallel.proposal_covariance(cfg, "SB2", 11).shape == (11, 11)
    for bad in ({"fit": [True, False]}, {"fit": [True, False], "tau": [INF, 3.0]}, {"fit": [True, False], "tau": [3.0, 3.0], "x": 1},
                {"fit": [True, False], "tau": [3.0, 3.0], "jumps": [1.0]}):
        with pytest.raises(ValueError):
            sample_parallel.timevar_block(dict(cfg, timevar=bad))


def test_posterior_refuses_injected_workers_with_time_scales():
    tv = {"fit": np.array([True, False]), "tau": np.array([25.0, INF])}
    with pytest.raises(ValueError, match="time scales need the library's own workers"):
        sample_parallel.Posterior("SB2", [], parameters=PARS, timevar=tv, make_worker=lambda ch: None)


def test_defects_of_the_batch_route_leave_the_value_bound_by_orders_of_magnitude():
    """tau read as (c, B), times not permuted with the pixels, the previous upload's tau kept: each moves lnp of some case by
    far more than the 1e-10 the GPU test allows -- measured on the float64 reference, no device"""
    import timevar_sampling_reference as tsr
    worst = {k: max(tsr.measure_defect(case, k) for case in tsr.CASES) for k in tsr.DEFECTS}
    print(worst)
    for k, v in worst.items():
        assert v >= 1e-4, (k, v)          # six orders of magnitude above the bound
    perm = [c for c in tsr.CASES if c.permuted]
    assert perm and tsr.measure_defect(perm[0], "times_not_permuted") >= 1e-4
    # and without a defect the same evaluation agrees with the long-double chain within the bound
    case = tsr.CASES[0]
    d = tsr.case_data(case)
    for b in (0, 8):
        want = tsr.chain_ext(case, b).lnp
        assert abs(tsr.lnp_f64(case, b, d.tau[b]) - want) <= 1e-10 * max(1.0, abs(want))
