"""Reference for the mixture moments (psoap_amd/csrc/mix_kernels.hpp): the law of total covariance over samples
s = 1 .. S with weights w_s, W = sum_s w_s, evaluated in NumPy long double from given (w_s, mu_s, Sigma_s):

    mu_mix    = sum_s w_s mu_s / W
    Sigma_mix = sum_s w_s Sigma_s / W  +  sum_s w_s (mu_s - mu_mix)(mu_s - mu_mix)^T / W        (within + between)

``moments`` is that evaluation (``dtype=np.float64``: the same statements in double, the yardstick of the GPU tolerances);
``DEFECTS`` are seeded wrong variants that tests/test_mix_reference.py must see rejected by sampling; ``derive_tolerances``
is the project's rule for the GPU tolerances; ``rpad`` / ``spad`` / ``upper_tiles`` / ``plan_bytes`` restate the padding rules
of mix_plan.hpp.  Run as a script it prints the tolerances of CPU stand-ins of the GPU cases."""
import numpy as np

NB, KB = 128, 16
MIX_MAX_S, MIX_MAX_R = 4096, 1 << 15


def rpad(R):
    return (R + NB - 1) // NB * NB


def spad(S):
    return (S + KB - 1) // KB * KB


def upper_tiles(Rt):
    """the launch order of k_mix_syrk: the upper triangle row-major"""
    return [(ti, tj) for ti in range(Rt) for tj in range(ti, Rt)]


def plan_bytes(R, S_max, want_sigma):
    Rp, Sp = rpad(R), spad(S_max)
    sbar = Rp * Rp if want_sigma else Rp
    out = Rp * Rp if want_sigma else 0
    return 8 * (sbar + out + 2 * Sp * Rp + Sp + 3 * Rp + 1)


def moments(w, mus, Sigmas, dtype=np.longdouble, defect=None):
    """-> dict mu (R,), Sigma (R, R), var_within (R,), var_between (R,), W.  ``Sigmas`` (S, R, R), or (S, R): variances only
    (``Sigma`` is then None).  ``defect``: one of ``DEFECTS``, a deliberately wrong evaluation."""
    w = np.asarray(w, dtype=dtype)
    mus = np.asarray(mus, dtype=dtype)
    Sg = np.asarray(Sigmas, dtype=dtype)
    S = w.shape[0]
    W = dtype(0)
    for s in range(S):
        W = W + w[s]
    norm = dtype(1) if defect == "unnormalised" else W
    acc = np.zeros(mus.shape[1], dtype=dtype)
    for s in range(S):
        acc = acc + w[s] * mus[s]
    mu = acc / norm
    centre = mus.mean(axis=0) if defect == "unweighted-centre" else mu
    within = np.zeros(Sg.shape[1:], dtype=dtype)
    for s in range(S):
        within = within + w[s] * Sg[s]
    within = within / norm
    full = Sg.ndim == 3
    between = np.zeros(Sg.shape[1:], dtype=dtype)
    if defect != "no-between":
        for s in range(S):
            d = mus[s] - centre
            between = between + (w[s] / norm) * (np.outer(d, d) if full else d * d)
    return {"mu": mu, "Sigma": within + between if full else None, "W": W,
            "var_within": np.diagonal(within).copy() if full else within,
            "var_between": np.diagonal(between).copy() if full else between}


DEFECTS = ("no-between", "unnormalised", "unweighted-centre")
OUTPUTS = ("mu", "Sigma", "var_within", "var_between")


def derive_tolerances(cases, factor=8.0):
    """The project's rule: per output, the largest deviation of the float64 evaluation from the long-double one over
    ``cases`` -- dicts ``w``, ``mus``, ``Sigmas``, ``scale`` (the largest prior variance of the case; the means are compared
    on its square root) -- relative to the scale, times ``factor``.  -> {output: relative tolerance}"""
    tol = dict.fromkeys(OUTPUTS, 0.0)
    for case in cases:
        ld = moments(case["w"], case["mus"], case["Sigmas"], np.longdouble)
        f64 = moments(case["w"], case["mus"], case["Sigmas"], np.float64)
        for k in OUTPUTS:
            if ld[k] is None:
                continue
            scale = np.sqrt(case["scale"]) if k == "mu" else case["scale"]
            dev = float(np.max(np.abs(f64[k].astype(np.longdouble) - ld[k]))) / float(scale)
            tol[k] = max(tol[k], factor * dev)
    return tol


def standin_case(R, S, seed, amp=0.2):
    """A CPU stand-in of a GPU case: S posteriors of a squared-exponential prior of variance amp^2 on R points, conditioned
    on noisy data at every fourth point with hyper-parameters jittered by a few percent per sample, unequal weights"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, R)
    obs = np.arange(0, R, 4)
    y = 0.1 * np.sin(9.0 * x[obs]) + 0.01 * rng.standard_normal(obs.shape[0])
    mus, Sigmas = [], []
    for _ in range(S):
        a, l = amp * (1.0 + 0.03 * rng.standard_normal()), 0.05 * (1.0 + 0.03 * rng.standard_normal())
        K = a * a * np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / (l * l))
        G = np.linalg.solve(K[np.ix_(obs, obs)] + 1e-4 * np.eye(obs.shape[0]), K[obs, :])
        mus.append(y @ G)
        Sg = K - K[:, obs] @ G
        Sigmas.append(0.5 * (Sg + Sg.T))
    return {"w": rng.uniform(0.5, 2.0, S), "mus": np.array(mus), "Sigmas": np.array(Sigmas), "scale": (1.03 * amp) ** 2 * 1.2}


# (R, S) of the GPU cases of tests/test_gpu_mix.py
GPU_SHAPES = [(128, 2), (129, KB - 1), (127, KB), (260, KB + 1), (128, KB + 1)]

if __name__ == "__main__":
    tol = derive_tolerances([standin_case(R, S, 100 + k) for k, (R, S) in enumerate(GPU_SHAPES)])
    for k in OUTPUTS:
        print(f"{k:12s} {tol[k]:.3e}")
