"""CPU: the references and the case list behind tests/test_gpu_forms.py.

* oracle.predict_f and oracle.predict_sum (c = 3) against the reference's own values at mu != 1 (golden_predict_f_v1.npz);
* the long-double references (oracle.lnlike_ext / predict_ext) against the LAPACK oracle;
* the case list declares every (form, scheme) cell of the persistent kernel, and the library builds no form more;
* every case can fail: dropping one tile update of its factorisation, or taking the wrong mean offset, moves the answer
  by at least 100x what the GPU test allows."""
import os
import sys

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import gpu_form_cases as fc

GOLDEN = os.path.join(fc.ROOT, "tests", "golden", "golden_predict_f_v1.npz")
sys.path.insert(0, os.path.dirname(GOLDEN))          # make_golden_predict_f: the inputs behind the golden's seeds


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def test_predict_f_matches_the_reference_at_every_prior_mean(oracle, gold):
    import make_golden_predict_f as mk
    for i, (ne, npx, seed, M, mu, amp, l) in enumerate(gold["pf_meta"]):
        ch, pred = mk.pf_inputs(int(ne), int(npx), int(seed), int(M))
        got_mu, got_S = oracle.predict_f(ch.lwls[0], ch.fl, ch.sigma, pred, amp, l, mu)
        assert np.max(np.abs(got_mu - gold[f"pf{i}_mu"])) <= 1e-12, i
        assert np.max(np.abs(got_S - gold[f"pf{i}_Sigma"])) <= 1e-12, i
    # the offset is the prior mean: the three means give three different answers
    assert np.max(np.abs(gold["pf0_mu"] - gold["pf1_mu"])) > 1e-3


def test_predict_sum_of_three_matches_the_reference_away_from_one(oracle, gold):
    import make_golden_predict_f as mk
    for i, (ne, npx, seed, mu) in enumerate(gold["ps_meta"]):
        ch, preds = mk.ps_inputs(int(ne), int(npx), int(seed))
        got_mu, got_S = oracle.predict_sum(ch.lwls, ch.fl, ch.sigma, preds, mu, [*fc.syn.GP_BASE[3]])
        assert np.max(np.abs(got_mu - gold[f"ps{i}_mu"])) <= 1e-12, i
        assert np.max(np.abs(got_S - gold[f"ps{i}_Sigma"])) <= 1e-12, i


@pytest.mark.parametrize("c,ne,npx,seed,mu", [(1, 3, 91, 1, 0.97), (2, 5, 51, 2, 1.0), (3, 2, 129, 3, 1.1)])
def test_long_double_lnlike_agrees_with_lapack(oracle, c, ne, npx, seed, mu):
    ch = fc.syn.make_chunk(c, ne, npx, seed=seed)
    gp = fc.syn.GP_BASE[c]
    ext = oracle.lnlike_ext(ch.lwls, ch.fl, ch.sigma, gp, mu)
    assert isinstance(ext, np.longdouble)
    lap = oracle.lnlike(ch.lwls, ch.fl, ch.sigma, gp, mu)
    assert abs(float(ext) - lap) <= 1e-12 * max(1.0, abs(lap))


@pytest.mark.parametrize("mode,c", [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 1)])
def test_long_double_predict_agrees_with_lapack(oracle, mode, c):
    ch = fc.syn.make_chunk(c, 3, 70, seed=40 + c)
    M = ch.N if (mode, c) == (1, 3) else 33
    pred = np.stack([np.linspace(w.min(), w.max(), M) for w in ch.lwls])
    mus = np.array([0.9, 0.2, -0.1][:c]) if mode == 0 else np.array([0.9])
    gp = np.array(fc.syn.GP_BASE[c])
    mu_x, S_x = oracle.predict_ext(mode, np.stack(ch.lwls), ch.fl, ch.sigma, pred, mus, gp)
    mu_l, S_l = fc.predict_lapack(mode, np.stack(ch.lwls), ch.fl, ch.sigma, pred, mus, gp)
    assert mu_x.dtype == np.longdouble
    assert np.max(np.abs(mu_x.astype(float) - mu_l)) <= 1e-12
    assert np.max(np.abs(S_x.astype(float) - S_l)) <= 1e-12


def test_the_case_list_declares_every_form_and_scheme():
    """39 cells: the 24 forms, the LAT and wide ones under schemes 1 and 2; a form the library gains without a case here
    fails (the library reports how many forms it builds)."""
    from psoap_amd import _lib
    assert len(fc.FORMS) == 24 and len(fc.CELLS) == 39
    assert _lib.load().psoap_dag_form_launches(None, 0) == len(fc.FORMS)
    assert tuple(_lib.DAG_FORM_NAMES) == fc.FORMS
    declared = {case.cell for case in fc.CASES}
    assert declared == set(fc.CELLS), sorted(set(fc.CELLS) ^ declared)
    names = [case.name for case in fc.CASES]
    assert len(set(names)) == len(names)
    # ragged tails, masked epochs, both covariance families, mu != 1; natural reach of a LAT and a TP cell
    Ns = [case.chunk().N for case in fc.CASES]
    assert {1, 16, 17, 127} <= {N % 128 for N in Ns} and sum(N % 16 != 0 for N in Ns) > len(Ns) // 2
    assert {case.family for case in fc.CASES} == {"base", "corr"} and any(case.masked for case in fc.CASES)
    assert all(case.mu != 1.0 for case in fc.CASES if case.kind != "predict")
    natural = {case.form for case in fc.CASES if case.kind == "lnlike" and not case.env}
    assert {"LAT", "TP"} <= natural
    # predict: modes 0, 1, 2 across C; predict_f (mode 2) at mu != 1
    assert {(case.mode, case.c) for case in fc.CASES if case.kind == "predict"} >= {(0, 1), (0, 2), (0, 3), (1, 2), (2, 1)}
    assert any(case.mode == 2 and case.mu != 1.0 for case in fc.CASES if case.kind == "predict")


# ---- sensitivity ------------------------------------------------------------------------------------------------------
def _blocked_lnp(K, r, drop=None, nb=128):
    """lnp through a right-looking blocked Cholesky in 128-wide tiles; drop = (i, j, k): skip the update of lower tile (i, j)
    by block column k (what a lost task of the persistent kernel would do)"""
    A = K.copy()
    n = A.shape[0]
    P = -(-n // nb)
    for k in range(P):
        k0, k1 = k * nb, min(n, (k + 1) * nb)
        A[k0:k1, k0:k1] = cholesky(A[k0:k1, k0:k1], lower=True)
        if k1 == n:
            break
        A[k1:, k0:k1] = solve_triangular(A[k0:k1, k0:k1], A[k1:, k0:k1].T, lower=True).T
        U = A[k1:, k0:k1] @ A[k1:, k0:k1].T
        if drop is not None and drop[2] == k:
            i, j = drop[0] * nb - k1, drop[1] * nb - k1
            U[i:i + nb, j:j + nb] = 0.0
            U[j:j + nb, i:i + nb] = 0.0
        A[k1:, k1:] -= U
    L = np.tril(A)
    z = solve_triangular(L, r, lower=True)
    return -0.5 * (z @ z + 2.0 * np.sum(np.log(np.diag(L))))


def _matrix(lwls, sigma, gp):
    import oracle
    lwls = np.atleast_2d(lwls)
    K = np.empty((lwls.shape[1],) * 2)
    oracle.fill_sym(K, lwls, gp)
    K[np.diag_indices_from(K)] += sigma ** 2
    return K


SENS = [case for case in fc.CASES if case.kind != "predict"]


@pytest.mark.parametrize("case", SENS, ids=[c.name for c in SENS])
def test_a_lost_tile_update_fails_the_case(oracle, case):
    """the last update of the last diagonal tile, and one of a far off-diagonal tile, each move lnp (of the first
    proposal, with the case's inputs) by >= 100x the contract tolerance the GPU test asserts"""
    ch, lw, gps, _ = fc.lnlike_inputs(case)
    K, r = _matrix(lw[0], ch.sigma, gps[0]), ch.fl - case.mu
    P = -(-ch.N // 128)
    assert P >= 2, "no tile update to lose"
    want = _blocked_lnp(K, r)
    assert abs(want - oracle.lnlike(lw[0], ch.fl, ch.sigma, gps[0], case.mu)) <= 1e-10 * max(1.0, abs(want))
    drops = [(P - 1, P - 1, P - 2)] + ([(P - 1, 1, 0)] if P >= 3 else [])
    for d in drops:
        try:
            bad = _blocked_lnp(K, r, drop=d)
        except np.linalg.LinAlgError:
            continue                        # the factorisation breaks down: fails on any tolerance
        assert not np.isfinite(bad) or abs(bad - want) >= 100 * fc.LNP_RTOL * max(1.0, abs(want)), (d, bad, want)


PSENS = [case for case in fc.CASES if case.kind == "predict" and
         fc.prediction_offset(case.mode, case.c, [case.mu]) != 1.0]


@pytest.mark.parametrize("case", PSENS, ids=[c.name for c in PSENS])
def test_the_wrong_mean_offset_fails_the_case(case):
    """mu at the offset the mode prescribes against mu with 1.0 in its place: apart by >= 100x the asserted atol"""
    ch, pred, mus = fc.predict_inputs(case)
    lw = np.stack(ch.lwls)
    right = fc.prediction_offset(case.mode, case.c, mus)
    mu_ok, _ = fc.predict_lapack(case.mode, lw, ch.fl, ch.sigma, pred, mus, case.gp())
    mu_bad, _ = fc.predict_lapack(case.mode, lw, ch.fl + (right - 1.0), ch.sigma, pred, mus, case.gp())
    assert np.max(np.abs(mu_ok - mu_bad)) >= 100 * fc.MU_ATOL


def test_the_wrong_mean_offset_fails_the_sum_of_three(gold):
    """predict_f_g_h_sum (mode 1, c = 3, the staged path) at the golden's mu != 1"""
    import make_golden_predict_f as mk
    for i, (ne, npx, seed, mu) in enumerate(gold["ps_meta"]):
        ch, preds = mk.ps_inputs(int(ne), int(npx), int(seed))
        gp = np.array(fc.syn.GP_BASE[3])
        bad, _ = fc.predict_lapack(1, np.stack(ch.lwls), ch.fl + (mu - 1.0), ch.sigma, preds, [mu], gp)
        assert np.max(np.abs(bad - gold[f"ps{i}_mu"])) >= 100 * fc.MU_ATOL
