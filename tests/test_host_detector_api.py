"""Photon and read-out noise of a detector (include/fastmpc.h: fmpc_detector), the parts that need no GPU: the library exports the
entry points, _lib.SIGNATURES binds them, the header declares them; every argument rule answers before the device is touched (the
pointers below are never dereferenced: each call is refused); the host read-out (fmpc_detector_read_host) against the numpy
restatement (tests/detector_ref.py) bit for bit; the accuracy of the draw's own exp and ln; the law of the Poisson deviate K --
moments, chi-square against scipy.stats.poisson, the third central moment --, its independence across measurements, realisations,
steps and of the normal draw of the same measurement; placement; and the reduction to FMPC_NOISE_SIGMA.

The statistical tests run on the HOST function with fixed seeds.  The device evaluates the same sequence of +, -, x, /, sqrt and
bit operations, and tests/test_gpu_detector.py holds it to the host's bits, so they vouch for what the GPU draws."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

from tests import detector_ref as dr

pkg = importlib.import_module("mpc-sensorlessao_amd")
_lib = pkg._lib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["fmpc_est_apply_detector_device", "fmpc_detector_read_device", "fmpc_detector_read_host", "fmpc_est_photon_gain"]
P = C.c_void_p(0x1000)                      # "some pointer": only ever passed to calls that are refused on their arguments
SEED = 20261020
SWITCH = 10.0                               # inversion below, PTRS from here on (csrc/fmpc_detector.h)
BELOW, ABOVE = 9.999, 10.001
LAMS = [0.0, 1e-3, BELOW, SWITCH, ABOVE, 30.0, 1e3, 1e6, 2.0 ** 31]


def block(gain=1.0, gain_dev=None, qe=1.0, background=0.0, read_noise=0.0, photon_noise=1, seed=SEED, step=0, step_dev=None, first=0):
    d = _lib.Detector()
    d.gain, d.gain_dev, d.qe, d.background, d.read_noise, d.photon_noise = gain, gain_dev, qe, background, read_noise, photon_noise
    d.seed, d.step, d.step_dev, d.first = seed, step, step_dev, first
    return d


def host_read(Y0, ld=0, out=None, **kw):
    lib = pkg.load()
    Y0 = np.ascontiguousarray(Y0, dtype=np.float64)
    batch, p = Y0.shape[0], (Y0.shape[1] if not ld else kw.pop("p"))
    if out is None:
        out = np.full_like(Y0, -7.0)
    d = block(**kw)
    assert lib.fmpc_detector_read_host(out.ctypes.data_as(C.c_void_p), Y0.ctypes.data_as(C.c_void_p), batch, p, ld, C.byref(d)) == _lib.FMPC_OK
    return out


def draws(lam, batch, p, **kw):
    """K(lam) over a (batch, p) grid: gain = 1, qe = 1, no background, no read-out noise."""
    return host_read(np.full((batch, p), lam), **kw)


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_bound_and_declared(name):
    lib = pkg.load()
    assert name in _lib.SIGNATURES
    fn = getattr(lib, name)
    assert fn.argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name


def test_python_layer_and_header_text():
    for name in ("DetectorNoise", "detector_read", "detector_read_host"):
        assert name in pkg.__all__ and getattr(pkg, name) is not None, name
    for name in ("photon_gain", "apply_device"):
        assert callable(getattr(pkg.PhaseDiversityEstimator, name))
    header = open(os.path.join(ROOT, "include", "fastmpc.h")).read()
    i = header.index("typedef struct fmpc_detector_s")
    text = header[header.rindex("/*", 0, i):i]
    for word in ("detector.m:315-321", "(a + 1) << 24", "2^31", "NaN", "folds it into the gain", "FMPC_E_DIM"):
        assert word in text, word
    # the struct as the header lays it out: double, pointer, three doubles, int, two 64-bit words, pointer, 64-bit word
    assert C.sizeof(_lib.Detector) == 80 and _lib.Detector.qe.offset == 16 and _lib.Detector.photon_noise.offset == 40
    assert _lib.Detector.seed.offset == 48 and _lib.Detector.first.offset == 72
    # the existing block keeps its layout
    assert C.sizeof(_lib.Noise) == 56 and _lib.Noise.value.offset == 8 and _lib.Noise.first.offset == 48
    d = pkg.DetectorNoise(2.5, read_noise=3.0, qe=0.8, background=4.0, seed=3, first=7)._block(step=2 ** 32 + 5)
    assert (d.gain, d.qe, d.background, d.read_noise, d.photon_noise, d.seed, d.step, d.first) == (2.5, 0.8, 4.0, 3.0, 1, 3, 2 ** 32 + 5, 7)
    assert not d.gain_dev and not d.step_dev
    assert pkg.DetectorNoise(1.0, photon_noise=False)._block().photon_noise == 0


NAN, INF = float("nan"), float("inf")
BAD = [dict(first=-1), dict(first=2 ** 32 - 2), dict(first=2 ** 32 + 1), dict(gain=-1.0), dict(gain=NAN), dict(gain=INF), dict(gain=0.0),
       dict(background=-1.0), dict(background=NAN), dict(background=INF), dict(read_noise=-1e-3), dict(read_noise=NAN), dict(read_noise=INF),
       dict(qe=0.0), dict(qe=-0.5), dict(qe=NAN), dict(qe=INF)]


def test_fused_call_argument_rules():
    lib = pkg.load()
    call = lambda e=P, batch=3, scrn=P, ad=P, **kw: lib.fmpc_est_apply_detector_device(e, batch, scrn, C.byref(block(**kw)), ad, None, None)
    assert call(e=None) == _lib.FMPC_E_NULL and call(ad=None) == _lib.FMPC_E_NULL and call(scrn=None) == _lib.FMPC_E_NULL
    assert lib.fmpc_est_apply_detector_device(P, 3, P, None, P, None, None) == _lib.FMPC_E_NULL
    for kw in BAD:
        assert call(**kw) == _lib.FMPC_E_DIM, kw
    assert call(batch=-1) == _lib.FMPC_E_DIM
    assert call(batch=0) == _lib.FMPC_OK                                                           # nothing to do: the handle is not read
    assert call(batch=0, qe=0.0) == _lib.FMPC_E_DIM                                                # ... but the block is judged
    assert call(batch=0, gain=0.0, gain_dev=0x1000) == _lib.FMPC_OK                                # gain == 0 is fine with gain_dev
    assert call(batch=2, first=2 ** 32 - 2, e=None) == _lib.FMPC_E_NULL
    assert call(batch=0, first=2 ** 32) == _lib.FMPC_OK and call(batch=1, first=2 ** 32) == _lib.FMPC_E_DIM
    g = C.c_double(-1.0)
    assert lib.fmpc_est_photon_gain(None, 1e3, C.byref(g)) == _lib.FMPC_E_NULL and lib.fmpc_est_photon_gain(P, 1e3, None) == _lib.FMPC_E_NULL
    for n in (0.0, -1.0, NAN, INF):
        assert lib.fmpc_est_photon_gain(P, n, C.byref(g)) == _lib.FMPC_E_DIM and g.value == -1.0, n


@pytest.mark.parametrize("where", ["device", "host"])
def test_read_argument_rules(where):
    lib = pkg.load()
    if where == "device":
        call = lambda Y=P, Y0=P, batch=3, p=50, ld=0, **kw: lib.fmpc_detector_read_device(Y, Y0, batch, p, ld, C.byref(block(**kw)), None)
        assert lib.fmpc_detector_read_device(P, P, 3, 50, 0, None, None) == _lib.FMPC_E_NULL
    else:
        call = lambda Y=P, Y0=P, batch=3, p=50, ld=0, **kw: lib.fmpc_detector_read_host(Y, Y0, batch, p, ld, C.byref(block(**kw)))
        assert lib.fmpc_detector_read_host(P, P, 3, 50, 0, None) == _lib.FMPC_E_NULL
        assert call(gain_dev=0x1000) == _lib.FMPC_E_DIM and call(step_dev=0x1000) == _lib.FMPC_E_DIM    # device pointers: not readable on the host
    assert call(Y=None) == _lib.FMPC_E_NULL and call(Y0=None) == _lib.FMPC_E_NULL
    for kw in BAD:
        assert call(**kw) == _lib.FMPC_E_DIM, kw
    assert call(batch=-1) == _lib.FMPC_E_DIM and call(p=0) == _lib.FMPC_E_DIM and call(p=-3) == _lib.FMPC_E_DIM
    assert call(p=2 ** 24 + 1) == _lib.FMPC_E_DIM                                                   # the counter layout's limit
    assert call(ld=49) == _lib.FMPC_E_DIM and call(ld=1) == _lib.FMPC_E_DIM and call(ld=-1) == _lib.FMPC_E_DIM
    assert call(batch=0) == _lib.FMPC_OK and call(batch=0, p=2 ** 24) == _lib.FMPC_OK


# ---- the restatement --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", LAMS)
def test_host_draw_against_the_restatement(lam):
    """4 000 draws per lam, bit for bit: both sides evaluate the same IEEE operations in the same order."""
    batch, p = 8, 500
    for seed, step, first in ((SEED, 0, 0), (0xF00DFACE12345678, 2 ** 32 + 5, 7)):
        got = draws(lam, batch, p, seed=seed, step=step, first=first)
        ref = dr.poisson(seed, step, first + np.arange(batch)[:, None], np.arange(p)[None, :], np.full((batch, p), lam))
        assert np.all(got == np.floor(got)) and np.all(got >= 0.0)
        assert np.array_equal(got, ref), (lam, seed, np.flatnonzero(got != ref)[:5])
    if lam == 0.0:
        assert np.all(got == 0.0)
    # and the Python wrapper is the same call
    assert np.array_equal(pkg.detector_read_host(np.full((batch, p), lam), pkg.DetectorNoise(1.0, seed=SEED)), draws(lam, batch, p))


def test_model_against_the_restatement_and_the_nan_domain():
    """The whole model on an array that spans every regime, with gain, qe and background: bit for bit against the restatement
    (the read-out term takes the library's own normal draw, so that two libms are not told apart).  lam < 0, above 2^31, NaN and inf
    give NaN, with and without photon noise; everything else is finite."""
    rng = np.random.default_rng(5)
    batch, p = 6, 700
    Y0 = 10.0 ** rng.uniform(-4, 9.2, (batch, p))
    Y0[:, ::50] = 0.0
    Y0[0, 1], Y0[1, 2], Y0[2, 3], Y0[3, 4], Y0[4, 5] = -1e-300, NAN, INF, -INF, 2.0 ** 33
    g = pkg.normal_noise_host(batch, p, pkg.EstimatorNoise(sigma=1.0, seed=SEED, first=3), step=4)
    for photon in (1, 0):
        for kw in (dict(gain=1.25), dict(gain=1.25, qe=0.7, read_noise=2.5), dict(gain=0.5, qe=0.9, background=3.0, read_noise=1.0)):
            got = host_read(Y0, photon_noise=photon, step=4, first=3, **kw)
            ref = dr.read(Y0, photon_noise=bool(photon), seed=SEED, step=4, first=3, normal=g, **kw)
            assert np.array_equal(got, ref, equal_nan=True), (photon, kw)
            bad = ~((kw["gain"] * Y0 + kw.get("background", 0.0) >= 0) & (kw["gain"] * Y0 + kw.get("background", 0.0) <= 2.0 ** 31))
            assert np.array_equal(np.isnan(got), bad) and bad.sum() >= 4
    # lam = 2^31 exactly is the last admissible value, the next double is not
    edge = host_read(np.array([[2.0 ** 30, 2.0 ** 30 * (1 + 2.0 ** -52), 0.0, -0.0]]), gain=2.0)
    assert np.isfinite(edge[0, 0]) and np.isnan(edge[0, 1]) and edge[0, 2] == 0.0 and edge[0, 3] == 0.0


def test_accuracy_of_the_own_exp_and_ln():
    """The draw's exp on [-10, 0] (exp(-lam) of the inversion) and ln on the ranges K uses it on -- a uniform in [2^-53, 1), lam and
    k in [10, 2^33], 1 / alpha in [1.12, 1.33], a / us^2 + b up to 1e37 -- on 10^4 points each: relative error <= 1e-13 against libm
    (a relative error eps there moves a probability by about eps)."""
    x = -np.linspace(0.0, 10.0, 10001)
    e = dr.det_exp(x)
    worst = max(abs(a - math.exp(b)) / math.exp(b) for a, b in zip(e, x))
    print(f"exp: worst relative error {worst:.2e}")
    assert worst <= 1e-13
    rng = np.random.default_rng(1)
    for lo, hi in ((2.0 ** -53, 1.0), (1.12, 1.33), (10.0, 2.0 ** 33), (1.0, 1e37), (0.999, 1.001)):
        v = np.exp(rng.uniform(np.log(lo), np.log(hi), 10000))
        v = v[v != 1.0]
        l = dr.det_ln(v)
        worst = max(abs(a - math.log(b)) / abs(math.log(b)) for a, b in zip(l, v))
        print(f"ln on [{lo:.3g}, {hi:.3g}]: worst relative error {worst:.2e}")
        assert worst <= 1e-13
    assert dr.det_ln(np.array([1.0]))[0] == 0.0 and dr.det_exp(np.array([-0.0]))[0] == 1.0
    # ln k! of the restatement: the table and the series against lgamma
    k = np.concatenate([np.arange(0, 200), 10.0 ** np.arange(3, 10)]).astype(np.float64)
    lf = dr.det_lnfact(k)
    assert max(abs(a - math.lgamma(b + 1.0)) / max(1.0, math.lgamma(b + 1.0)) for a, b in zip(lf, k)) <= 1e-14


# ---- the law ----------------------------------------------------------------------------------------------------------------
def _chi2(x, lam):
    """Pearson's statistic against scipy.stats.poisson: integer bins between the 1e-4 quantiles with the tails merged until the
    expected count is >= 20; where that is more than 400 bins, 64 bins at the law's quantiles.  Returns (statistic, df)."""
    from scipy import stats
    N = x.size
    law = stats.poisson(lam)
    lo, hi = int(law.ppf(1e-4)), int(law.ppf(1.0 - 1e-4))
    if hi - lo + 1 > 400:
        edges = np.unique(law.ppf(np.arange(1, 64) / 64.0))                # bins (-inf, e0], (e0, e1], .., (e_last, inf)
        cdf = np.concatenate([[0.0], law.cdf(edges), [1.0]])
        expected = N * np.diff(cdf)
        observed = np.bincount(np.searchsorted(edges, x, side="left"), minlength=edges.size + 1).astype(np.float64)
    else:
        ks = np.arange(lo, hi + 1)
        expected = N * law.pmf(ks)
        expected[0] = N * law.cdf(lo)
        expected[-1] = N * law.sf(hi - 1)
        observed = np.bincount(np.clip(x, lo, hi).astype(np.int64) - lo, minlength=ks.size).astype(np.float64)
        # from either tail inward: bins are joined until the group expects >= 20; what is left over joins the bin of the mode
        im = int(np.argmax(expected))

        def walk(e, o):
            ge, go, ae, ao = [], [], 0.0, 0.0
            for a, b in zip(e, o):
                ae, ao = ae + a, ao + b
                if ae >= 20.0:
                    ge.append(ae); go.append(ao)
                    ae, ao = 0.0, 0.0
            return ge, go, ae, ao
        le, lo_, lre, lro = walk(expected[:im], observed[:im])
        re_, ro, rre, rro = walk(expected[:im:-1], observed[:im:-1])
        expected = np.array(le + [expected[im] + lre + rre] + re_[::-1])
        observed = np.array(lo_ + [observed[im] + lro + rro] + ro[::-1])
    assert observed.sum() == N and abs(expected.sum() - N) <= 1e-6 * N and expected.min() >= 20.0 and expected.size >= 2
    return float(((observed - expected) ** 2 / expected).sum()), expected.size - 1


@pytest.mark.parametrize("lam", [1e-3, 0.5, 3.0, BELOW, ABOVE, 30.0, 1e3, 1e6, 2.0 ** 31])
def test_law_of_the_draw(lam):
    """N = 2e5 draws of the host function over a (100, 2000) grid at a fixed seed: |mean - lam| <= 6 sqrt(lam / N); |s^2 - lam| <=
    6 sqrt((lam + 2 lam^2) / N) (the variance of a sample variance is (mu_4 - sigma^4) / N, mu_4 = lam + 3 lam^2); chi-square below
    chi2.isf(1e-6, df).  numpy's own sampler sits at 0.02 - 0.19 of the moment bars and well under every chi-square threshold with
    this binning.  A bar that trips is a finding about K, not a reason to change the seed."""
    from scipy import stats
    batch, p = 100, 2000
    N = batch * p
    x = draws(lam, batch, p)
    m, v = x.mean(), x.var(ddof=1)
    bm, bv = 6 * np.sqrt(lam / N), 6 * np.sqrt((lam + 2 * lam ** 2) / N)
    c2, df = _chi2(x.ravel(), lam)
    thr = stats.chi2.isf(1e-6, df)
    print(f"lam {lam:g}: mean {abs(m - lam) / bm:.3f} of its bar, variance {abs(v - lam) / bv:.3f} of its bar, chi2 {c2:.1f} at df {df} (threshold {thr:.1f})")
    assert abs(m - lam) <= bm and abs(v - lam) <= bv
    assert c2 <= thr


def test_third_central_moment():
    """lam = 1e3, N = 2e6: |m_3 - lam| <= 6 sqrt(15 lam^3 / N).  The law's skewness is 11 standard errors of m_3 there, so a rounded
    normal -- whose third moment vanishes -- fails this.  Above lam of about 1e4 no feasible test tells the two laws apart (the
    skewness falls below the standard error of any sample of <= 1e7 draws): there the exactness of K rests on the algorithm, the
    accuracy of its exp and ln, and the chi-square tests above."""
    lam, batch, p = 1e3, 1000, 2000
    N = batch * p
    x = draws(lam, batch, p, seed=SEED + 1)
    m3 = ((x - x.mean()) ** 3).mean()
    bar = 6 * np.sqrt(15 * lam ** 3 / N)
    print(f"m3 = {m3:.1f} for {lam:g}: {abs(m3 - lam) / bar:.3f} of its bar ({bar:.1f})")
    assert abs(m3 - lam) <= bar


def _corr(a, b):
    return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])


@pytest.mark.parametrize("lam", [3.0, 30.0])
def test_independence(lam):
    """Correlation of K at (R, i) and (R, i + 1), at (R, i) and (R + 1, i), at step and step + 1, and of K - lam with the normal
    draw g of the same (seed, step, R, i) -- the condition on the counter layout: no Philox block serves both -- each <= 6 / sqrt N
    in magnitude, N = 2e5; one lam in either regime."""
    batch, p = 100, 2000
    N = batch * p
    x = draws(lam, batch, p, step=3)
    x1 = draws(lam, batch, p, step=4)
    g = pkg.normal_noise_host(batch, p, pkg.EstimatorNoise(sigma=1.0, seed=SEED), step=3)
    pairs = {"measurement": (x[:, :-1], x[:, 1:]), "realisation": (x[:-1], x[1:]), "step": (x, x1), "normal draw": (x - lam, g)}
    for name, (a, b) in pairs.items():
        c = _corr(a, b)
        print(f"lam {lam:g}, across {name}: correlation {c * np.sqrt(N):+.2f} / sqrt N")
        assert abs(c) <= 6 / np.sqrt(N), name
    # the halves of the seed and of the step matter
    for kw in (dict(step=3 + 2 ** 32), dict(seed=SEED + 1), dict(seed=SEED + 2 ** 32), dict(first=1)):
        assert not np.array_equal(draws(lam, 2, p, step=kw.pop("step", 3), **kw), x[:2]), kw


# ---- placement, reduction ---------------------------------------------------------------------------------------------------
def test_placement_is_bitwise():
    """A realisation's row is the same alone, in a batch of 5 through `first`, and with ld > p, where the padding -- of Y0 as of Y --
    is untouched; in place (Y == Y0) as well."""
    rng = np.random.default_rng(2)
    p = 301
    Y0 = 10.0 ** rng.uniform(-2, 5, (5, p))
    kw = dict(gain=2.0, qe=0.9, background=1.5, read_noise=1.0, step=3)
    for f in (0, 7, 2 ** 32 - 5):
        full = host_read(Y0, first=f, **kw)
        assert np.all(np.isfinite(full))
        for r in range(5):
            assert np.array_equal(full[r], host_read(Y0[r:r + 1], first=f + r, **kw)[0]), (f, r)
    pad_in = np.full((5, 320), NAN)
    pad_in[:, :p] = Y0
    pad_out = np.full((5, 320), -7.0)
    host_read(pad_in, ld=320, p=p, out=pad_out, **kw)
    assert np.array_equal(pad_out[:, :p], host_read(Y0, **kw)) and np.all(pad_out[:, p:] == -7.0)
    host_read(pad_in, ld=320, p=p, out=pad_in, **kw)                                              # in place
    assert np.array_equal(pad_in[:, :p], pad_out[:, :p]) and np.all(np.isnan(pad_in[:, p:]))


def test_reduction_to_sigma():
    """photon_noise = 0, background = 0, qe = 1, gain = 1: bitwise Y0 + fmpc_noise_normal_host(sigma = read_noise) -- the
    products by 1 and the sums with 0 are exact, and the read-out term is rounded as FMPC_NOISE_SIGMA rounds it."""
    rng = np.random.default_rng(3)
    batch, p = 4, 2883
    Y0 = np.abs(rng.standard_normal((batch, p))) * 10.0 ** rng.uniform(-6, 3, (batch, p))
    for rn in (0.37, 1e-3, 0.0):
        for step, first in ((0, 0), (2 ** 32 + 5, 7)):
            got = host_read(Y0, photon_noise=0, read_noise=rn, step=step, first=first)
            ref = Y0 + pkg.normal_noise_host(batch, p, pkg.EstimatorNoise(sigma=rn, seed=SEED, first=first), step=step)
            assert np.array_equal(got, ref), (rn, step)
    assert not np.array_equal(host_read(Y0, photon_noise=0, read_noise=0.37), Y0)
