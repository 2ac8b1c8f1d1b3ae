"""GPU tests of the mixture moments (psoap_chunk_mix_begin / _add / _finish / _release; psoap_amd/csrc/mix_kernels.hpp,
mix_plan.hpp) and of the Python layers on top (ChunkHandle.mix_*, covariance.predict_mixture, retrieve.retrieve_posterior).

Shapes: N = 120 .. 240 (three or four epochs of psoap_amd.synthetic), the benchmark hyper-parameters jittered by 3 % and the
velocities by 0.2 km/s per sample, unequal weights in [0.5, 2]; (c, M) across the 128-tile edges -- (2, 64) R = 128,
(3, 43) R = 129, (1, 127) R = 127 in mode 2, (2, 130) R = 260: three upper tiles with a mirror --, mode 1 once, and
S in {1, 2, 15, 16, 17} around the tile engine's K stage of 16.

Exact checks are bit for bit.  Every other comparison is against tests/mix_reference.py (long double) fed with the mu_s,
Sigma_s that psoap_chunk_predict downloads, to the DERIVED tolerance: per output the largest deviation of the float64 NumPy
evaluation from the long-double one over these cases, relative to the largest prior variance (its square root for the mean),
times 8 -- nothing fitted to the device's results.  Derived and device-measured values: DESIGN.md section 3h."""
import ctypes
import functools

import numpy as np
import pytest

import mix_reference as mr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

KB = mr.KB
# name -> (c, M, mode, n_epochs, n_pix, S)
CASES = {"R128-S2": (2, 64, 0, 4, 50, 2), "R129-S15": (3, 43, 0, 3, 40, KB - 1), "R127-S16": (1, 127, 2, 4, 60, KB),
         "R260-S17": (2, 130, 0, 4, 50, KB + 1), "sum-R128-S17": (2, 128, 1, 4, 50, KB + 1)}
NO_MIX = "no mixture on this handle"


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the chunk, the prediction grid and the S samples of a case"""
    c, M, mode, ne, npx, S = CASES[name]
    ch = syn.make_chunk(c, ne, npx, seed=7300 + 10 * c + S)
    rng = np.random.default_rng(900 + S + 100 * c)
    lwls = syn.walker_lwls(ch, syn.make_walker_velocities(ch, S, seed=31 + S))
    gps = np.array(syn.GP_BASE[c]) * (1.0 + 0.03 * rng.standard_normal((S, 2 * c)))
    w = rng.uniform(0.5, 2.0, S)
    pred = np.stack([np.linspace(ch.lwls[0].min(), ch.lwls[0].max(), M)] * c)
    mus = [0.0] * c if mode == 0 else [1.0]
    amp2 = gps[:, 0::2] ** 2
    scale = float(np.max(amp2) if mode == 0 else np.max(amp2.sum(axis=1)) + 1e-8)      # the largest prior variance
    return {"ch": ch, "lwls": lwls, "gps": gps, "w": w, "pred": pred, "mus": mus, "mode": mode, "S": S, "scale": scale,
            "R": c * M if mode == 0 else M}


def _handle(ch, sigma=None):
    from psoap_amd.chunk import ChunkHandle
    return ChunkHandle(ch.fl, ch.sigma if sigma is None else sigma)


def _mix(h, inp, order=None, want_sigma=True, weights=None, marg=False):
    order = range(inp["S"]) if order is None else order
    w = inp["w"] if weights is None else weights
    h.mix_begin(inp["mode"], inp["pred"], inp["mus"], len(order), want_sigma=want_sigma, marg=marg)
    for s in order:
        assert h.mix_add(inp["lwls"][s], inp["gps"][s], w[s])
    return h.mix_finish()


@functools.lru_cache(maxsize=None)
def device(name):
    """one handle per case, once per session: the predictions of every sample by psoap_chunk_predict, the mixture (finished
    twice), the variance-only mixture, the adds in reverse order"""
    inp = inputs(name)
    S = inp["S"]
    with _handle(inp["ch"]) as h:
        per = [h.predict(inp["mode"], inp["lwls"][s], inp["pred"], inp["mus"], inp["gps"][s]) for s in range(S)]
        per_var = [h.predict(inp["mode"], inp["lwls"][s], inp["pred"], inp["mus"], inp["gps"][s], want_sigma="diag") for s in range(S)]
        full = _mix(h, inp)
        again = h.mix_finish()
        var = _mix(h, inp, want_sigma=False)
        rev = _mix(h, inp, order=list(range(S))[::-1])
        h.mix_release()
    assert all(_same_bits(p[0], q[0]) for p, q in zip(per, per_var))
    return {"mus": np.array([p[0] for p in per]), "Sigmas": np.array([p[1] for p in per]), "vars": np.array([q[1] for q in per_var]),
            "full": full, "again": again,
            "var": var, "rev": rev}


@functools.lru_cache(maxsize=None)
def reference(name):
    inp, dev = inputs(name), device(name)
    return mr.moments(inp["w"], dev["mus"], dev["Sigmas"])


@functools.lru_cache(maxsize=None)
def tolerances():
    """the project's rule over the GPU cases (mix_reference.derive_tolerances)"""
    cases = [{"w": inputs(n)["w"], "mus": device(n)["mus"], "Sigmas": device(n)["Sigmas"], "scale": inputs(n)["scale"]} for n in CASES]
    tol = mr.derive_tolerances(cases)
    print("derived tolerances:", {k: f"{v:.3e}" for k, v in tol.items()})
    return tol


@functools.lru_cache(maxsize=None)
def tolerances_var():
    """the same rule for the variance-only mode: the cases fed with the variances psoap_chunk_predict_var downloads"""
    cases = [{"w": inputs(n)["w"], "mus": device(n)["mus"], "Sigmas": device(n)["vars"], "scale": inputs(n)["scale"]} for n in CASES]
    tol = mr.derive_tolerances(cases)
    print("derived tolerances, variance-only:", {k: f"{v:.3e}" for k, v in tol.items()})
    return tol


def _deviation(name, got, want, key):
    inp = inputs(name)
    scale = np.sqrt(inp["scale"]) if key == "mu" else inp["scale"]
    return float(np.max(np.abs(got[key].astype(np.longdouble) - want[key]))) / scale


# ---- against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_mixture_against_the_long_double_reference(name):
    tol, dev, ref, inp = tolerances(), device(name), reference(name), inputs(name)
    got = dev["full"]
    assert got["n_folded"] == inp["S"] and got["Sigma"].shape == (inp["R"], inp["R"])
    assert float(ref["W"]) == pytest.approx(got["W"], rel=1e-15)
    for key in mr.OUTPUTS:
        d = _deviation(name, got, ref, key)
        print(f"{name} {key}: deviation {d:.3e} of the scale, tolerance {tol[key]:.3e}")
    for key in mr.OUTPUTS:
        assert _deviation(name, got, ref, key) <= tol[key], key
    # diag(Sigma) = var_within + var_between
    d = float(np.max(np.abs(np.diag(got["Sigma"]) - (got["var_within"] + got["var_between"])))) / inp["scale"]
    print(f"{name} diag(Sigma) - (within + between): {d:.3e}")
    assert d <= tol["Sigma"]


@pytest.mark.parametrize("name", list(CASES))
def test_symmetry_and_second_finish_are_exact(name):
    dev = device(name)
    assert _same_bits(dev["full"]["Sigma"], dev["full"]["Sigma"].T.copy())
    for key in ("mu", "Sigma", "var_within", "var_between"):
        assert _same_bits(dev["full"][key], dev["again"][key]), key
    assert dev["full"]["W"] == dev["again"]["W"] and dev["again"]["n_folded"] == inputs(name)["S"]


@pytest.mark.parametrize("name", list(CASES))
def test_variance_only_mode(name):
    """Against the reference fed with what this mode folds: the variances psoap_chunk_predict_var downloads.  Against the full
    mode's diagonal the inputs themselves differ -- var_s = prior - column norms^2 and diag(Sigma_s) round differently inside
    the predict calls -- and a weighted mean of the inputs moves by at most the largest of those differences: the bound is that
    difference plus the derived tolerances of both modes."""
    tol, tolv, dev, inp = tolerances(), tolerances_var(), device(name), inputs(name)
    var = dev["var"]
    ref = mr.moments(inp["w"], dev["mus"], dev["vars"])
    assert var["Sigma"] is None and var["n_folded"] == inp["S"]
    assert _same_bits(var["mu"], dev["full"]["mu"]), "mu differs between want_sigma 0 and 1"
    for key in ("mu", "var_within", "var_between"):
        d = _deviation(name, var, ref, key)
        print(f"{name} variance-only {key}: deviation {d:.3e}, tolerance {tolv[key]:.3e}")
        assert d <= tolv[key], key
    inputs_differ = float(np.max(np.abs(dev["vars"] - np.array([np.diag(S) for S in dev["Sigmas"]])))) / inp["scale"]
    bound = inputs_differ + tol["var_within"] + tol["var_between"] + tolv["var_within"] + tolv["var_between"]
    d = float(np.max(np.abs(var["var_within"] + var["var_between"] - np.diag(dev["full"]["Sigma"])))) / inp["scale"]
    print(f"{name} variance-only against the full mode's diagonal: {d:.3e}, inputs differ by {inputs_differ:.3e}, bound {bound:.3e}")
    assert d <= bound
    assert _same_bits(var["var_between"], dev["full"]["var_between"]) or _deviation(name, var, reference(name), "var_between") <= tol["var_between"]


@pytest.mark.parametrize("name", list(CASES))
def test_reordered_adds_agree_to_tolerance(name):
    tol, dev, ref = tolerances(), device(name), reference(name)
    for key in mr.OUTPUTS:
        d = _deviation(name, dev["rev"], ref, key)
        print(f"{name} reversed adds {key}: deviation {d:.3e}, tolerance {tol[key]:.3e}")
        assert d <= tol[key], key


# ---- exact checks -----------------------------------------------------------------------------------------------------------
BASELINE = {"order": 1, "sd": [0.05, 0.02]}


@pytest.mark.parametrize("marg", [False, True], ids=["plain", "marg"])
def test_one_sample_of_weight_one_is_the_predict_call(marg):
    inp = inputs("R260-S17")
    ch = inp["ch"]
    with _handle(ch) as h:
        if marg:
            h.set_baseline(BASELINE["order"], ch.lwl, ch.epoch_index, ch.n_epochs, BASELINE["sd"])
        call = h.predict_marg if marg else h.predict
        mu, Sigma = call(inp["mode"], inp["lwls"][3], inp["pred"], inp["mus"], inp["gps"][3])
        _, var = call(inp["mode"], inp["lwls"][3], inp["pred"], inp["mus"], inp["gps"][3], want_sigma="diag")
        one = _mix(h, inp, order=[3], weights=np.ones(inp["S"]), marg=marg)
        assert _same_bits(one["mu"], mu) and _same_bits(one["Sigma"], Sigma)
        assert not one["var_between"].any() and _same_bits(one["var_within"], np.diag(Sigma).copy())
        assert (one["n_folded"], one["W"]) == (1, 1.0)
        # the same sample twice with weight 1: the same bits again
        two = _mix(h, inp, order=[3, 3], weights=np.ones(inp["S"]), marg=marg)
        assert _same_bits(two["mu"], mu) and _same_bits(two["Sigma"], Sigma) and not two["var_between"].any()
        assert (two["n_folded"], two["W"]) == (2, 2.0)
        # variance-only: the _var twin's bits
        v1 = _mix(h, inp, order=[3], weights=np.ones(inp["S"]), want_sigma=False, marg=marg)
        assert _same_bits(v1["mu"], mu) and _same_bits(v1["var_within"], var) and not v1["var_between"].any()


def test_finish_between_adds_equals_a_fresh_mixture_and_predict_between_adds_disturbs_nothing():
    inp = inputs("R129-S15")
    k = 4
    with _handle(inp["ch"]) as h:
        alone = h.predict(inp["mode"], inp["lwls"][9], inp["pred"], inp["mus"], inp["gps"][9])
        h.mix_begin(inp["mode"], inp["pred"], inp["mus"], inp["S"])
        for s in range(k):
            assert h.mix_add(inp["lwls"][s], inp["gps"][s], inp["w"][s])
        part = h.mix_finish()
        between = h.predict(inp["mode"], inp["lwls"][9], inp["pred"], inp["mus"], inp["gps"][9])
        assert _same_bits(between[0], alone[0]) and _same_bits(between[1], alone[1])
        h.predict_release()                       # the mixture's buffers are its own
        for s in range(k, inp["S"]):
            assert h.mix_add(inp["lwls"][s], inp["gps"][s], inp["w"][s])
        whole = h.mix_finish()
        fresh = _mix(h, inp, order=list(range(k)))
    assert part["n_folded"] == k and whole["n_folded"] == inp["S"]
    for key in ("mu", "Sigma", "var_within", "var_between", "W"):
        assert _same_bits(np.asarray(part[key]), np.asarray(fresh[key])), key
        assert _same_bits(np.asarray(whole[key]), np.asarray(device("R129-S15")["full"][key])), key


def test_a_sample_that_is_not_positive_definite_is_skipped():
    """zero noise on the first pixel and a sample with zero amplitudes: its first pivot is exactly 0 -> status 1"""
    inp = inputs("R128-S2")
    ch = inp["ch"]
    sigma = ch.sigma.copy()
    sigma[0] = 0.0
    bad_gp = inp["gps"][0].copy()
    bad_gp[0::2] = 0.0
    with _handle(ch, sigma) as h:
        with pytest.raises(np.linalg.LinAlgError):
            h.predict(inp["mode"], inp["lwls"][0], inp["pred"], inp["mus"], bad_gp)
        for want in (True, False):
            clean = _mix(h, inp, want_sigma=want)
            h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 3, want_sigma=want)
            assert h.mix_add(inp["lwls"][0], inp["gps"][0], inp["w"][0])
            assert not h.mix_add(inp["lwls"][0], bad_gp, 1.7)
            assert h.mix_add(inp["lwls"][1], inp["gps"][1], inp["w"][1])
            got = h.mix_finish()
            assert got["n_folded"] == 2
            for key in ("mu", "var_within", "var_between", "W") + (("Sigma",) if want else ()):
                assert _same_bits(np.asarray(got[key]), np.asarray(clean[key])), (want, key)
    from psoap_amd import covariance as cov
    res = cov.predict_mixture([inp["lwls"][0], inp["lwls"][0], inp["lwls"][1]], ch.fl, sigma, inp["pred"], inp["mus"],
                              [inp["gps"][0], bad_gp, inp["gps"][1]], weights=[inp["w"][0], 1.7, inp["w"][1]])
    assert res["skipped"] == [1] and res["n_folded"] == 2
    cov.release_handles()


def test_draws_after_an_add_are_the_draws_after_the_plain_predict():
    inp = inputs("R129-S15")
    with _handle(inp["ch"]) as h:
        h.predict(inp["mode"], inp["lwls"][2], inp["pred"], inp["mus"], inp["gps"][2])
        want = h.predict_draw(3, seed=11)
        h.predict(inp["mode"], inp["lwls"][5], inp["pred"], inp["mus"], inp["gps"][5])
        h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 4)
        assert h.mix_add(inp["lwls"][2], inp["gps"][2], 0.7)
        got = h.predict_draw(3, seed=11)
        assert _same_bits(got, want)
        # a variance-only add leaves no Sigma to draw from
        h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 4, want_sigma=False)
        assert h.mix_add(inp["lwls"][2], inp["gps"][2], 0.7)
        from psoap_amd._lib import PsoapError
        with pytest.raises(PsoapError, match="no predict call has formed Sigma"):
            h.predict_draw(3, seed=11)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from psoap_amd._lib import PsoapError
    inp = inputs("R128-S2")
    ch = inp["ch"]
    a = (inp["lwls"][0], inp["gps"][0])
    with _handle(ch) as h:
        with pytest.raises(PsoapError, match="psoap_chunk_mix_add: " + NO_MIX):
            h.mix_add(*a)
        with pytest.raises(PsoapError, match="psoap_chunk_mix_finish: " + NO_MIX):
            h.mix_finish()
        for s_max, msg in ((0, "S_max must be at least 1"), (mr.MIX_MAX_S + 1, "S_max must be at most 4096")):
            with pytest.raises(PsoapError, match="psoap_chunk_mix_begin: " + msg):
                h.mix_begin(inp["mode"], inp["pred"], inp["mus"], s_max)
        with pytest.raises(PsoapError, match="psoap_chunk_mix_begin: .*baseline"):
            h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 2, marg=True)
        h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 2)
        with pytest.raises(PsoapError, match="psoap_chunk_mix_finish: no sample has been folded yet") as e:
            h.mix_finish()
        assert "rc=2" in str(e.value)
        for w in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(PsoapError, match="psoap_chunk_mix_add: weight must be finite and > 0"):
                h.mix_add(*a, w)
        assert h.mix_add(*a) and h.mix_add(*a)
        with pytest.raises(PsoapError, match="psoap_chunk_mix_add: the mixture already holds S_max samples"):
            h.mix_add(*a)
        assert h.mix_finish()["n_folded"] == 2
        # an open stream
        h.stream_open(2, 1)
        try:
            for call in (lambda: h.mix_add(*a), h.mix_finish, lambda: h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 2)):
                with pytest.raises(PsoapError, match="open stream"):
                    call()
        finally:
            h.stream_close()
        assert h.mix_finish()["n_folded"] == 2
        # what ends a mixture; psoap_chunk_predict_release does not
        h.predict_release()
        assert h.mix_finish()["n_folded"] == 2
        h.set_data(ch.fl, ch.sigma)
        with pytest.raises(PsoapError, match="psoap_chunk_mix_finish: " + NO_MIX):
            h.mix_finish()
        h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 2)
        assert h.mix_add(*a)
        h.set_baseline(BASELINE["order"], ch.lwl, ch.epoch_index, ch.n_epochs, BASELINE["sd"])
        with pytest.raises(PsoapError, match="psoap_chunk_mix_add: " + NO_MIX):
            h.mix_add(*a)
        h.mix_begin(inp["mode"], inp["pred"], inp["mus"], 2, want_sigma=False)
        assert h.mix_add(*a)
        with pytest.raises(PsoapError, match="Sigma_out must be NULL in the variance-only mode"):
            h.mix_finish(want_sigma=True)
        h.mix_release()
        with pytest.raises(PsoapError, match="psoap_chunk_mix_finish: " + NO_MIX):
            h.mix_finish()


# ---- the Python layers --------------------------------------------------------------------------------------------------------
def _chunk2d(s):
    from psoap_amd import data as pdata

    def full(v, fill):
        out = np.full(s.mask.shape, fill)
        out[s.mask] = v
        return out
    date = np.broadcast_to(s.dates[:, None], s.mask.shape).copy()
    return pdata.Chunk(np.exp(full(s.lwl, 8.5)), full(s.fl, 1.0), full(s.sigma, 1.0), date, s.mask.copy())


def test_retrieve_posterior(tmp_path):
    from psoap_amd import covariance as cov
    from psoap_amd import retrieve
    from psoap_amd.utils import convert_dict, registered_params
    s = syn.make_chunk(2, 4, 40, seed=8801, masked_fraction=0.05)
    p_orb = syn.make_orbit_proposals("SB2", 1, seed=8802)[0]
    pars = dict(zip(registered_params["SB2"], list(p_orb) + list(syn.GP_BASE[2])))
    fix = ["gamma"]
    p0 = convert_dict("SB2", fix, **pars)
    base = retrieve.retrieve_components("SB2", _chunk2d(s), pars)
    # one chain row equal to the point estimate: retrieve_components, bit for bit
    one = retrieve.retrieve_posterior("SB2", _chunk2d(s), pars, p0[None, :], fix, n_samples=1)
    assert one["n_folded"] == 1 and one["skipped"] == []
    for key in ("wl_predict", "lwl_predict", "mu", "Sigma", "lwls", "mu_f", "mu_g", "sigma_f", "sigma_g"):
        assert _same_bits(one[key], base[key]), key
    assert not one["sigma_between_f"].any() and _same_bits(one["sigma_within_g"], base["sigma_g"])
    # five rows against the host composition of five retrieve_components calls on the fixed grid
    rng = np.random.default_rng(8803)
    chain = p0[None, :] * (1.0 + 0.01 * rng.standard_normal((5, p0.shape[0])))
    post = retrieve.retrieve_posterior("SB2", _chunk2d(s), pars, chain, fix, n_samples=64, draws_per_sample=2, seed=40)
    assert post["n_folded"] == 5 and list(post["rows"]) == [0, 1, 2, 3, 4]
    M = base["lwl_predict"].shape[0]
    mus, Sigmas, scale = [], [], 0.0
    for row in chain:
        pr = dict(pars)
        pr.update(dict(zip([n for n in registered_params["SB2"] if n not in fix], row)))
        # (retrieve_components takes its own grid at ITS parameters: the sample's grids, the point estimate's prediction grid)
        lw = retrieve.retrieve_components("SB2", _chunk2d(s), pr, get_Sigma=False)["lwls"]
        gp = [pr[n] for n in registered_params["SB2"][7:]]
        mu_s, Sig_s = cov.predict_f_g(lw[0], lw[1], s.fl, s.sigma, base["lwl_predict"], base["lwl_predict"], 0.0, gp[0], gp[1], 0.0,
                                      gp[2], gp[3])
        mus.append(mu_s)
        Sigmas.append(Sig_s)
        scale = max(scale, gp[0] ** 2, gp[2] ** 2)
    case = {"w": np.ones(5), "mus": np.array(mus), "Sigmas": np.array(Sigmas), "scale": scale}
    tol = mr.derive_tolerances([case])
    ref = mr.moments(case["w"], case["mus"], case["Sigmas"])
    for key in mr.OUTPUTS:
        got = {"mu": post["mu"], "Sigma": post["Sigma"],
               "var_within": np.concatenate([post["sigma_within_f"], post["sigma_within_g"]]) ** 2,
               "var_between": np.concatenate([post["sigma_between_f"], post["sigma_between_g"]]) ** 2}[key]
        d = float(np.max(np.abs(got.astype(np.longdouble) - ref[key]))) / (np.sqrt(scale) if key == "mu" else scale)
        # (the variances went through sqrt and a square on the way: two more roundings of the value itself)
        slack = 4 * 2.0 ** -53 if key.startswith("var") else 0.0
        print(f"retrieve_posterior {key}: deviation {d:.3e}, tolerance {tol[key]:.3e} + {slack:.1e}")
        assert d <= tol[key] + slack, key
    assert np.all(post["sigma_between_g"] > 0) and np.all(post["sigma_g"] >= post["sigma_within_g"])
    assert post["f_draws"].shape == (10, M) and post["g_draws"].shape == (10, M)
    retrieve.save_components(post, str(tmp_path / "plots"))
    f = np.load(tmp_path / "plots" / "f.npy")
    assert f.shape == (3, M) and np.array_equal(f[1], post["mu_f"]) and np.array_equal(f[2], post["sigma_f"])
    assert (tmp_path / "plots" / "Sigma.npy").exists() and (tmp_path / "plots" / "g_draws.npy").exists()
    diag = retrieve.retrieve_posterior("SB2", _chunk2d(s), pars, chain, fix, get_Sigma="diag")
    assert diag["Sigma"] is None and _same_bits(diag["mu"], post["mu"])
    cov.release_handles()
