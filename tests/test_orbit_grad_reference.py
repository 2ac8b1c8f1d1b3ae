"""CPU checks that pin the formulas of tests/orbit_grad_reference.py -- and with them what the device is held to in
tests/test_gpu_orbit_grad.py: the long-double Jacobian against long-double central differences of
``orbit_ext.velocities_ext``, seeded defects against that same check, the chain against central differences of the oracle's
``lnlike`` through ``orbit_ext``, and the ``ChunkWorker`` plumbing with the handle call replaced."""
import numpy as np
import pytest

import grad_reference as gr
import orbit_cases as oc
import orbit_ext as oe
import orbit_grad_reference as ogr
from psoap_amd import synthetic as syn

_LD = np.longdouble
FD_BOUND = 1e-5            # of S_J: the step sets the floor (7.4e-7 of |J| on an SB2 orbit with e = 0.6, P = 23, T0 = 2455010)
SUBSET_E = (0.0, 0.5, 0.79, 0.95, 0.99)

pytestmark = pytest.mark.skipif(not oe.have_ext(), reason=oe.skip_reason())


def _orbit_of(model, k):
    """(base name, orbit suffix) of parameter k"""
    name = oc.NAMES[model][k]
    base, _, orb = name.partition("_")
    return base, ("_" + orb if orb else "")


def _step(model, p, k):
    """1e-7 max(1, |p_k|); 1e-10 |p_k| for P and T0; the step in e scaled by (1 - e)"""
    base, _ = _orbit_of(model, k)
    if base in ("P", "T0"):
        return 1e-10 * abs(p[k])
    h = 1e-7 * max(1.0, abs(p[k]))
    return h * (1.0 - p[k]) if base == "e" else h


def _difference_is_valid(model, p, k, h, dates):
    """Where a central difference with step h can resolve the derivative at all -- a property of the DIFFERENCE, decided from
    the parameters and the dates alone, never from the Jacobian under test.  Only P and T0 have such places:

    * the step moves the mean anomaly by dM = 2 pi h |t - T0| / P^2 (P) or 2 pi h / P (T0), the eccentric anomaly by dM / D,
      D = 1 - e cos E; near periastron f varies on the scale sqrt(D) of E, so the truncation of the central difference is
      about dM^2 / (6 D^3) of the derivative: dates with dM^2 / D^3 > 1e-6 are left out (e >= 0.85 at a periastron passage);
    * dv/dP is proportional to t - T0: at |t - T0| < P / 1000 (the table's dates one ulp from T0) the derivative vanishes
      while the reference's own double phase reduction moves tt by ulps of P between the two points."""
    base, orb = _orbit_of(model, k)
    if base not in ("P", "T0"):
        return np.ones(len(dates), dtype=bool)
    names = oc.NAMES[model]
    T0, P, e = (p[names.index(n + orb)] for n in ("T0", "P", "e"))
    dt = np.abs(dates - T0)
    dM = 2 * np.pi * h * (dt / P ** 2 if base == "P" else 1.0 / P)
    E = np.asarray(oe.eccentric_anomaly(oe.mean_anomaly(dates, T0, P), e), dtype=np.float64)
    D = 1.0 - e * np.cos(E)
    ok = dM ** 2 / D ** 3 <= 1e-6
    return ok & (dt >= 1e-3 * P) if base == "P" else ok


def _central_differences(model, p, dates):
    """(D (c, n, n_orb), valid (n, n_orb)) by long-double central differences; a zero step (T0 == 0) is not valid"""
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros((oc.N_COMPONENTS[model], len(dates), len(p)), dtype=_LD)
    valid = np.zeros((len(dates), len(p)), dtype=bool)
    for k in range(len(p)):
        h = _step(model, p, k)
        if h == 0.0:
            continue
        hi, lo = p.copy(), p.copy()
        hi[k] += h
        lo[k] -= h
        if _orbit_of(model, k)[0] == "e" and lo[k] < 0.0:        # e = 0: the half-line
            lo[k] = p[k]
        out[:, :, k] = (oe.velocities_ext(model, hi, dates) - oe.velocities_ext(model, lo, dates)) / (_LD(hi[k]) - _LD(lo[k]))
        valid[:, k] = _difference_is_valid(model, p, k, h, dates)
    return out, valid


def _subset():
    """(case, row) pairs: the eccentricity ladder at SUBSET_E for every model and orbit, every _PHASE_CONFIGS pair (its e = 0.3
    and 0.99 rows: the dates reach 4.9e6 periods from T0) and the q rows of the role cases"""
    picks = []
    for case in oc.VEL_CASES:
        tag = case.tags[0]
        if tag == "ecc" and case.model in ("SB1", "SB2", "ST3"):
            picks += [(case, i) for i, e in enumerate(oc.E_LADDER) if e in SUBSET_E]
        elif tag == "ecc":
            picks += [(case, 2)]
        elif tag == "phase" and (case.model == "SB2" or case.name.startswith("phase-ST3_out-P3.7123")):
            picks += [(case, 1), (case, 3)]
        elif tag == "roles" and case.model in ("SB2", "ST2", "ST3"):
            n_om = len(oc._OMEGAS) * len(oc.ORBITS[case.model])
            picks += [(case, i) for i in range(n_om, len(case.P))] + [(case, 1), (case, 5)]
    return picks


def _worst_disagreement(jacobian, picks):
    """largest |J - D| / S_J over the valid entries (S_J from the reference)"""
    worst = 0.0
    for case, i in picks:
        p = case.P[i]
        D, valid = _central_differences(case.model, p, case.dates)
        J, _ = jacobian(case.model, p, case.dates)
        _, S = ogr.jacobian_ext(case.model, p, case.dates)
        ok = valid[None] & (S > 0)
        if not np.all(J[S == 0] == 0):              # a structural zero that is not one
            return np.inf
        if ok.any():
            worst = max(worst, float(np.max(np.abs(J - D)[ok] / S[ok])))
    return worst


_SUBSET = None


def _picks():
    global _SUBSET
    if _SUBSET is None:
        _SUBSET = _subset()
    return _SUBSET


def test_subset_spans_what_it_should():
    picks = _picks()
    models = {case.model for case, _ in picks}
    assert models == set(oc.MODELS)
    es, pairs, qs, far = set(), set(), set(), 0.0
    for case, i in picks:
        p, names = case.P[i], oc.NAMES[case.model]
        for orb in oc.ORBITS[case.model]:
            es.add(p[names.index("e" + orb)])
            pairs.add((p[names.index("P" + orb)], p[names.index("T0" + orb)]))
            far = max(far, float(np.max(np.abs(case.dates - p[names.index("T0" + orb)]) / p[names.index("P" + orb)])))
        qs.update(p[names.index(n)] for n in names if n.startswith("q"))
    assert set(SUBSET_E) <= es and set(oc._PHASE_CONFIGS) <= pairs and set(oc._QS) <= qs and far > 1e6


def test_long_double_jacobian_matches_central_differences():
    worst = _worst_disagreement(ogr.jacobian_ext, _picks())
    print(f"largest |J - D| / S_J over the subset: {worst:.2e} (bound {FD_BOUND:.0e})")
    assert worst <= FD_BOUND


def test_valid_differences_cover_every_parameter_and_most_dates():
    """the validity rule leaves out little: every parameter of every model is compared at some date, P and T0 included"""
    kept = total = 0
    for case, i in _picks():
        p = case.P[i]
        for k in range(len(p)):
            h = _step(case.model, p, k)
            if h == 0.0:
                continue
            v = _difference_is_valid(case.model, p, k, h, case.dates)
            kept, total = kept + int(v.sum()), total + v.size
            if _orbit_of(case.model, k)[0] not in ("P", "T0"):
                assert v.all()
    assert kept >= 0.9 * total


@pytest.mark.parametrize("defect", ogr.JAC_DEFECTS)
def test_seeded_defects_are_rejected(defect):
    """a restated Jacobian with one defect fails the check that the reference passes"""
    picks = [(c, i) for c, i in _picks() if c.tags[0] in ("ecc", "roles") and (defect != "st3_in_out_swapped" or c.model == "ST3")]
    worst = _worst_disagreement(lambda m, p, d: ogr.jacobian_ext(m, p, d, defect=defect), picks[:12] + picks[-12:])
    print(f"{defect}: {worst:.2e}")
    assert worst > 100 * FD_BOUND


def test_float64_jacobian_agrees_with_long_double():
    """what TOL_J of tests/test_gpu_orbit_grad.py is derived from, on a corner of the table"""
    case = next(c for c in oc.VEL_CASES if c.name == "roles-ST3")
    for p in case.P[:4]:
        Je, Se = ogr.jacobian_ext(case.model, p, case.dates)
        Jf, _ = ogr.jacobian_f64(case.model, p, case.dates)
        assert ogr.rel_to_scale(Jf, Je, Se) < 1e-12
    # structural zeros: ST3's tertiary does not depend on the inner orbit
    assert np.all(Je[2, :, :6] == 0) and np.all(Je[0, :, [0, 6]] == 0) and np.all(Je[1, :, 6] == 0)


# ---- the chain ----------------------------------------------------------------------------------------------------------
def _chain_chunk(model):
    c = oc.N_COMPONENTS[model]
    full = syn.make_chunk(c, 6, 14, seed=6200 + c)
    keep = np.sort(np.random.default_rng(6300 + c).choice(6 * 14, size=60, replace=False))
    mask = np.zeros(6 * 14, dtype=bool)
    mask[keep] = True
    mask = mask.reshape(6, 14)
    assert len(set(mask.sum(axis=1))) > 1
    return full.lwl[keep], full.fl[keep], full.sigma[keep], syn.epoch_index_from_mask(mask), full.dates


@pytest.mark.parametrize("model", ["SB1", "SB2", "ST3"])
def test_chain_matches_finite_differences_of_the_oracle(oracle, model):
    """Central differences of ``oracle.lnlike`` (float64) on grids made by ``orbit_ext`` around ORBIT_BASE, N = 60 in 6
    unequal epochs; the step and the bound are those of tests/test_grad_reference.py for grad_lwl, moved to the parameter:
    the ln-wavelengths move by |J| h / c_kms, which is held at that file's 2e-8 for the fastest-moving pixel; the bound is
    truncation (|D(2h) - D(h)| 2/3 from the long-double likelihood, below 1e-6 of S_orb) + the oracle's rounding measured at
    the two points + 1e-12 S_orb.  One term is new here: both likelihoods take the shifted grids rounded to double, which
    moves every pixel by up to half an ulp of its ln-wavelength at each of the two points, and the difference by up to
    sum_ci |dlnL/dlwl_ci| ulp(lwl) / 2h."""
    lwl, fl, sigma, ep, dates = _chain_chunk(model)
    p0, gp, mu = np.array(syn.ORBIT_BASE[model]), np.array(syn.GP_BASE[oc.N_COMPONENTS[model]]), gr.MU_GP
    ref = ogr.chain_from(model, p0, gp, lwl, fl, sigma, ep, dates, mu)
    J, _ = ogr.jacobian_ext(model, p0, dates)
    grid_rounding = float(np.sum(np.abs(ref.grad.lwl))) * float(np.spacing(np.max(lwl)))

    def grids(p):
        return np.asarray(oe.shift_ext(lwl, oe.velocities_ext(model, p, dates), ep), dtype=np.float64)

    for k in range(len(p0)):
        h = 2e-8 * oe.C_KMS / float(np.max(np.abs(J[:, :, k])))

        def at(d, k=k):
            p = p0.copy()
            p[k] += d
            return grids(p)
        f_or = lambda d: _LD(oracle.lnlike(at(d), fl, sigma, gp, mu))              # noqa: E731
        f_ext = lambda d: oracle.lnlike_ext(at(d), fl, sigma, gp, mu)              # noqa: E731
        cd = lambda f, s: (f(+s) - f(-s)) / (2 * s)                                 # noqa: E731
        d1, d2 = cd(f_ext, h), cd(f_ext, 2 * h)
        trunc = 2 * abs(d2 - d1) / 3
        scale = ref.s_orb[k]
        assert trunc <= 1e-6 * scale, (k, float(trunc), float(scale))
        noise = (abs(f_or(+h) - f_ext(+h)) + abs(f_or(-h) - f_ext(-h))) / (2 * h)
        got, bound = cd(f_or, h), trunc + noise + 1e-12 * scale + grid_rounding / (2 * h)
        print(f"{oc.NAMES[model][k]:10s} analytic {float(ref.orb[k]):+.9e} difference {float(got):+.9e} bound {float(bound):.2e}")
        assert abs(got - ref.orb[k]) <= bound, (oc.NAMES[model][k], float(ref.orb[k]), float(got), float(bound))


def test_chain_cases_have_the_sizes_the_tiles_need():
    assert sorted((c.model, c.N) for c in ogr.CHAIN_CASES) == [("SB1", 300), ("SB2", 129), ("SB2", 300), ("ST1", 128), ("ST3", 300)]
    for case in ogr.CHAIN_CASES:
        ch = case.chunk
        assert ch.N == case.N and len(set(ch.mask.sum(axis=1))) > 1 and len(ch.dates) == case.n_epochs


# ---- ChunkWorker plumbing without a device ------------------------------------------------------------------------------
class _FakeHandle:
    def __init__(self):
        self.calls = []

    def lnprob_grad(self, model_id, p_orb, gps, mu_GP=1.0, want_vel=False):
        self.calls.append((model_id, p_orb.copy(), gps.copy(), mu_GP))
        B = p_orb.shape[0]
        g_orb = 100.0 + np.arange(p_orb.shape[1])[None] + 1000.0 * np.arange(B)[:, None]
        g_gp = 200.0 + np.arange(gps.shape[1])[None] + 1000.0 * np.arange(B)[:, None]
        return np.arange(B, dtype=float), g_orb, g_gp, np.zeros(B)


def _worker(model, fix_params=(), defaults=None):
    from psoap_amd.lnprob import ChunkWorker
    w = ChunkWorker.__new__(ChunkWorker)
    w.model, w.fix_params, w.defaults, w.handle = model, list(fix_params), dict(defaults or {}), _FakeHandle()
    return w


def test_worker_selects_the_fitted_entries_in_registered_order(monkeypatch):
    monkeypatch.delenv("PSOAP_GPU_SERVER", raising=False)
    from psoap_amd.utils import registered_params
    fix = ["e", "gamma", "l_g"]
    w = _worker("SB2", fix, {"e": 0.1, "gamma": 3.0, "l_g": 7.0})
    reg = registered_params["SB2"]
    n_fit = len(reg) - len(fix)
    ps = np.arange(2 * n_fit, dtype=float).reshape(2, n_fit) + 1.0
    lnp, grad = w.lnprob_grad_batch(ps, mu_GP=0.9)
    assert lnp.shape == (2,) and grad.shape == (2, n_fit)
    model_id, p_orb, gps, mu = w.handle.calls[0]
    assert model_id == 1 and p_orb.shape == (2, 7) and gps.shape == (2, 4) and mu == 0.9
    assert p_orb[0, 2] == 0.1 and p_orb[1, 6] == 3.0 and gps[0, 3] == 7.0
    want = [(100.0 + i if i < 7 else 200.0 + i - 7) for i, name in enumerate(reg) if name not in fix]
    assert np.array_equal(grad[0], want) and np.array_equal(grad[1], np.array(want) + 1000.0)
    one_lnp, one_grad = w.lnprob_grad(ps[0])
    assert isinstance(one_lnp, float) and one_grad.shape == (n_fit,) and np.array_equal(one_grad, want)
    # nothing fixed: the whole vector
    w = _worker("ST3")
    lnp, grad = w.lnprob_grad_batch(np.ones((3, 19)))
    assert grad.shape == (3, 19) and np.array_equal(grad[0], np.concatenate([100.0 + np.arange(13), 200.0 + np.arange(6)]))


def test_worker_refuses_fitted_st2_vectors_and_takes_split_ones(monkeypatch):
    monkeypatch.delenv("PSOAP_GPU_SERVER", raising=False)
    w = _worker("ST2")
    with pytest.raises(ValueError):                       # two registered GP parameters, a likelihood of two components
        w.lnprob_grad_batch(np.ones((1, 14)))
    assert not w.handle.calls
    lnp, g_orb, g_gp, g_mu = w.lnprob_grad_orbits(np.ones((2, 12)), np.ones((2, 4)))
    assert g_orb.shape == (2, 12) and g_gp.shape == (2, 4) and lnp.shape == g_mu.shape == (2,)
    with pytest.raises(ValueError):
        w.lnprob_grad_orbits(np.ones((2, 11)), np.ones((2, 4)))


def test_worker_refuses_under_the_gpu_server(monkeypatch):
    from psoap_amd._lib import PsoapError
    monkeypatch.setenv("PSOAP_GPU_SERVER", "auto")
    w = _worker("SB1")
    with pytest.raises(PsoapError, match="serves values only"):
        w.lnprob_grad(np.ones(8))
    assert not w.handle.calls


def test_optimize_orbit_sums_the_workers_and_hands_scipy_the_gradient():
    """two quadratic 'chunks': the fit lands on the minimum of their SUM, a non-finite value is (inf, zeros)"""
    from psoap_amd.lnprob import optimize_orbit

    class Quad:
        def __init__(self, centre):
            self.centre, self.n = np.asarray(centre, dtype=float), 0

        def lnprob_grad(self, p, mu_GP=1.0):
            self.n += 1
            if p[0] > 50.0:
                return -np.inf, np.full_like(p, np.nan)
            return float(-0.5 * np.sum((p - self.centre) ** 2)), -(p - self.centre)

    a, b = Quad([1.0, 2.0]), Quad([3.0, -2.0])
    res = optimize_orbit([a, b], [0.0, 0.0], full_output=True)
    assert res.success and np.allclose(res.x, [2.0, 0.0], atol=1e-6) and a.n == b.n > 0
    assert np.allclose(optimize_orbit([a, b], [0.5, 0.5], bounds=[(0.0, 1.0), (None, None)]), [1.0, 0.0], atol=1e-6)
