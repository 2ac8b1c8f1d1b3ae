"""The long-double reference of the mixture moments (tests/mix_reference.py) pinned to sampling: for a 3-sample mixture of
small Gaussians (R = 4) the empirical mean and covariance of 2e6 seeded draws FROM THE MIXTURE -- a component by its weight,
then a vector from that component's Gaussian -- agree with ``moments`` within their Monte-Carlo standard errors, and each
seeded defect (the between term left out, weights not normalised, centring on the unweighted mean) is rejected by the same
bound.  Then the rule that derives the GPU tolerances, on CPU stand-ins of the GPU cases."""
import numpy as np
import pytest

import mix_reference as mr

N_DRAWS = 2_000_000
N_SE = 5.0      # standard errors allowed (fixed seed: the run is deterministic; 5 sigma over 14 numbers is 1e-5 by chance)


@pytest.fixture(scope="module")
def mixture():
    rng = np.random.default_rng(20260117)
    R = 4
    w = np.array([0.5, 1.5, 3.0])                      # unequal, W = 5: not normalised
    mus = np.array([[0.0, 1.0, -1.0, 2.0], [1.5, -0.5, 0.5, 0.0], [-1.0, 0.2, 1.2, -0.7]])
    Sigmas = []
    for s in range(3):
        A = 0.4 * rng.standard_normal((R, R))
        Sigmas.append(A @ A.T + 0.05 * (s + 1) * np.eye(R))
    Sigmas = np.array(Sigmas)
    comp = rng.choice(3, size=N_DRAWS, p=w / w.sum())
    x = np.empty((N_DRAWS, R))
    for s in range(3):
        idx = np.nonzero(comp == s)[0]
        x[idx] = mus[s] + rng.standard_normal((idx.shape[0], R)) @ np.linalg.cholesky(Sigmas[s]).T
    mean = x.mean(axis=0)
    d = x - mean
    cov = d.T @ d / N_DRAWS
    # standard errors: of the mean sqrt(var / n); of cov_ij sqrt((E[d_i^2 d_j^2] - cov_ij^2) / n)
    se_mean = np.sqrt(np.diag(cov) / N_DRAWS)
    m4 = np.einsum("ni,nj->ij", d * d, d * d) / N_DRAWS
    se_cov = np.sqrt((m4 - cov * cov) / N_DRAWS)
    return {"w": w, "mus": mus, "Sigmas": Sigmas, "mean": mean, "cov": cov, "se_mean": se_mean, "se_cov": se_cov}


def _worst(m, got):
    """the largest deviation from the empirical moments in units of their standard errors: (mean, covariance)"""
    zm = np.max(np.abs(np.asarray(got["mu"], dtype=np.float64) - m["mean"]) / m["se_mean"])
    zc = np.max(np.abs(np.asarray(got["Sigma"], dtype=np.float64) - m["cov"]) / m["se_cov"])
    return zm, zc


def test_reference_agrees_with_mixture_draws(mixture):
    got = mr.moments(mixture["w"], mixture["mus"], mixture["Sigmas"])
    zm, zc = _worst(mixture, got)
    print(f"mean: {zm:.2f} standard errors, covariance: {zc:.2f}")
    assert zm < N_SE and zc < N_SE
    # the parts: diag(Sigma) = var_within + var_between, and the variance-only form gives the same diagonals
    assert np.allclose(np.diag(got["Sigma"]).astype(float), (got["var_within"] + got["var_between"]).astype(float), rtol=1e-15)
    var = mr.moments(mixture["w"], mixture["mus"], np.array([np.diag(S) for S in mixture["Sigmas"]]))
    assert var["Sigma"] is None
    for k in ("mu", "var_within", "var_between"):
        assert np.allclose(var[k].astype(float), got[k].astype(float), rtol=1e-15)
    assert float(got["W"]) == 5.0


@pytest.mark.parametrize("defect", mr.DEFECTS)
def test_seeded_defects_are_rejected(mixture, defect):
    got = mr.moments(mixture["w"], mixture["mus"], mixture["Sigmas"], defect=defect)
    zm, zc = _worst(mixture, got)
    print(f"{defect}: mean {zm:.1f} standard errors, covariance {zc:.1f}")
    assert max(zm, zc) > 10 * N_SE


def test_float64_evaluation_is_close_and_single_sample_is_exact(mixture):
    ld = mr.moments(mixture["w"], mixture["mus"], mixture["Sigmas"])
    f64 = mr.moments(mixture["w"], mixture["mus"], mixture["Sigmas"], np.float64)
    assert f64["Sigma"].dtype == np.float64
    assert np.max(np.abs(f64["Sigma"] - ld["Sigma"].astype(float))) < 1e-14
    one = mr.moments([1.0], mixture["mus"][:1], mixture["Sigmas"][:1], np.float64)
    assert np.array_equal(one["mu"], mixture["mus"][0]) and np.array_equal(one["Sigma"], mixture["Sigmas"][0])
    assert not one["var_between"].any()


def test_tolerance_rule_on_standins_of_the_gpu_cases():
    cases = [mr.standin_case(R, S, 100 + k) for k, (R, S) in enumerate(mr.GPU_SHAPES[:3])]
    tol = mr.derive_tolerances(cases)
    print({k: f"{v:.2e}" for k, v in tol.items()})
    # a few units of 2^-53 times 8: no wider than 1e-13, and not zero (the float64 evaluation does round)
    for k in mr.OUTPUTS:
        assert 0.0 < tol[k] < 1e-13, (k, tol[k])
    assert mr.derive_tolerances(cases, factor=16.0)["Sigma"] == 2.0 * tol["Sigma"]
    # a single sample of weight 1 leaves nothing to round
    one = [{"w": [1.0], "mus": cases[0]["mus"][:1], "Sigmas": cases[0]["Sigmas"][:1], "scale": cases[0]["scale"]}]
    assert set(mr.derive_tolerances(one).values()) == {0.0}


def test_padding_twin():
    assert [mr.rpad(R) for R in (1, 127, 128, 129, 256, 3072)] == [128, 128, 128, 256, 256, 3072]
    assert [mr.spad(S) for S in (1, 15, 16, 17, 4096)] == [16, 16, 16, 32, 4096]
    assert mr.upper_tiles(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert mr.plan_bytes(3072, 64, 1) == 8 * (2 * 3072 * 3072 + 2 * 64 * 3072 + 64 + 3 * 3072 + 1)
