"""GPU tests of the detector's photon and read-out noise (include/fastmpc.h: fmpc_detector, fmpc_est_apply_detector_device,
fmpc_detector_read_device).  Estimators and screens are those of tests/test_gpu_est_noise.py.  The law of the Poisson deviate is
tested on the host function (tests/test_host_detector_api.py); here the device is held to the host's bits, and the fused call to
the composition of the calls it fuses:
  1. the stand-alone call against the host call over every regime of the draw: bit for bit without read-out noise (the device's /,
     sqrt and the draw's own exp and ln agree with the host's), 1e-12 read_noise / gain with it (the normal draw's two libms);
  2. fused against composed at every kernel form: Y_out bit for bit, ad_est to a bar from the test's own data;
  3. the reduction to FMPC_NOISE_SIGMA, bit for bit;  4. independence of position in the batch, and across the boundary between
     the few-screen and the general finish;  5. the counter on the device under a graph;  6. AOLoop.step with a DetectorNoise.
Every test prints the worst figure it saw."""
import numpy as np
import pytest

from tests.test_gpu_est_noise import SHAPES, _estimator, _dev, _np

pytestmark = pytest.mark.gpu

SEED = 20261020
EPS = 2.2e-16
NAN, INF = float("nan"), float("inf")


def _lam_array():
    """(8, 12500) expected counts: a quarter each log-uniform over [1e-4, 10), [10, 1e3), [1e3, 1e6), [1e6, 2^31], then the
    marked values: 0, both sides of the switch point of the draw (10), 2^31 and what lies outside the domain."""
    rng = np.random.default_rng(7)
    batch, p = 8, 12500
    lo = np.array([1e-4, 10.0, 1e3, 1e6])[np.arange(batch * p) % 4]
    hi = np.array([10.0, 1e3, 1e6, 2.0 ** 31])[np.arange(batch * p) % 4]
    lam = np.exp(rng.uniform(np.log(lo), np.log(hi))).reshape(batch, p)
    marked = [0.0, -0.0, 9.999, np.nextafter(10.0, 0.0), 10.0, 10.001, 2.0 ** 31, np.nextafter(2.0 ** 31, 0.0), 2.0 ** -1074, 15.0, 16.0, 17.0]
    outside = [-1.0, -1e-300, NAN, INF, -INF, np.nextafter(2.0 ** 31, INF), 1e300]
    for r in range(batch):
        lam[r, 100 * r:100 * r + len(marked)] = marked
        lam[r, 6000 + 100 * r:6000 + 100 * r + len(outside)] = outside
    return lam, len(outside) * batch


# ---- 1. the stand-alone call against the host call --------------------------------------------------------------------------
def test_read_device_against_host(pkg, gpu):
    import torch
    lam, n_out = _lam_array()
    batch, p = lam.shape
    d_lam = _dev(lam)
    checked = 0
    for seed, step, first in ((SEED, 0, 0), (0xF00DFACE12345678, 2 ** 32 + 5, 7)):
        det = pkg.DetectorNoise(1.0, seed=seed, first=first)
        got = _np(pkg.detector_read(d_lam, det, step=step))
        ref = pkg.detector_read_host(lam, det, step=step)
        assert np.isnan(ref).sum() == n_out and np.all(ref[~np.isnan(ref)] >= 0.0)
        assert np.array_equal(got, ref, equal_nan=True), np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5]
        checked += got.size
    # gain, qe, background: still bit for bit without read-out noise (lam = gain Y0 + background on either side)
    Y0 = lam / 1.25
    det = pkg.DetectorNoise(1.25, qe=0.7, background=3.0, seed=SEED, first=2)
    got, ref = _np(pkg.detector_read(_dev(Y0), det, step=1)), pkg.detector_read_host(Y0, det, step=1)
    assert np.array_equal(got, ref, equal_nan=True) and np.isnan(ref).sum() >= n_out - 2 * batch     # (-1e-300 and -1 + 3 are inside now)
    # with read-out noise: the normal draw goes through two libms
    worst = 0.0
    for gain, rn, photon in ((1.25, 3.0, True), (0.5, 1.0, False), (0.25, 10.0, True)):
        det = pkg.DetectorNoise(gain, photon_noise=photon, read_noise=rn, qe=0.9, background=2.0, seed=SEED, first=5)
        got, ref = _np(pkg.detector_read(_dev(Y0), det, step=3)), pkg.detector_read_host(Y0, det, step=3)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        ok = ~np.isnan(ref)
        w = np.abs(got[ok] - ref[ok]).max() / (rn / gain)
        worst = max(worst, w)
        assert w <= 1e-12, (gain, rn, photon, w)
    print(f"1. ({batch}, {p}): {checked} draws bit for bit; with read-out noise worst {worst:.2e} read_noise / gain")
    # in place, and ld > p with the padding untouched (of the input and of the output)
    det = pkg.DetectorNoise(1.25, read_noise=3.0, background=2.0, seed=SEED)
    plain = _np(pkg.detector_read(_dev(Y0), det, step=2))
    buf = _dev(Y0)
    assert pkg.detector_read(buf, det, step=2, out=buf) is buf and np.array_equal(_np(buf), plain, equal_nan=True)
    wide_in = torch.full((batch, p + 13), NAN, dtype=torch.float64, device=gpu)
    wide_in[:, :p] = _dev(Y0)
    wide_out = torch.full((batch, p + 13), -7.0, dtype=torch.float64, device=gpu)
    pkg.detector_read(wide_in[:, :p], det, step=2, out=wide_out[:, :p])
    o = _np(wide_out)
    assert np.array_equal(o[:, :p], plain, equal_nan=True) and np.all(o[:, p:] == -7.0)
    # a realisation's row does not depend on the batch it sits in; gain from the device; the counter on the device
    assert np.array_equal(_np(pkg.detector_read(_dev(Y0[3:5]), pkg.DetectorNoise(1.25, read_noise=3.0, background=2.0, seed=SEED, first=3), step=2)), plain[3:5], equal_nan=True)
    gains = np.full(batch, 1.25)
    assert np.array_equal(_np(pkg.detector_read(_dev(Y0), pkg.DetectorNoise(_dev(gains), read_noise=3.0, background=2.0, seed=SEED), step=2)), plain, equal_nan=True)
    ctr = torch.tensor([2], dtype=torch.int64, device=gpu)
    assert np.array_equal(_np(pkg.detector_read(_dev(Y0), pkg.DetectorNoise(1.25, read_noise=3.0, background=2.0, seed=SEED, counter=ctr), step=0)), plain, equal_nan=True)


def test_photon_gain(pkg, gpu):
    """gain = n_photons ndiv / sum(b_s), against the test's own b_s; with it the unaberrated image holds n_photons ndiv electrons."""
    for name in ("len64_d31", "len64_d5_two"):
        (est, D, A_s, b_s), _ = _estimator(pkg, name)
        for n in (1e3, 1e6, 2.5):
            g = est.photon_gain(n)
            assert abs(g - n * est.ndiv / b_s.sum()) <= 2 * est.p * EPS * g and abs(g * b_s.sum() / est.ndiv - n) <= 4 * est.p * EPS * n
        for n in (0.0, -1.0, NAN, INF):
            with pytest.raises(pkg.FastMPCError) as e:
                est.photon_gain(n)
            assert e.value.code == pkg._lib.FMPC_E_DIM


# ---- 2. fused against composed ----------------------------------------------------------------------------------------------
def _ad_bar(G, Y, Y0, b_s, p):
    """2 p eps sum_i |G_ji| (|Y_i - b_i| + |Y0_i - b_i|) per component: fixed-order sums of p terms on either side."""
    return 2 * p * EPS * ((np.abs(Y - b_s) + np.abs(Y0 - b_s)) @ np.abs(G).T)


@pytest.mark.parametrize("name", list(SHAPES))
def test_fused_equals_composed(pkg, gpu, name):
    (est, D, A_s, b_s), scr = _estimator(pkg, name)
    batch, p = SHAPES[name][5], est.p
    s = _dev(scr[:batch])
    G = np.linalg.pinv(A_s.T @ A_s) @ A_s.T
    ad0, Y0 = est.apply_device(s, want_Y=True)
    ad0_h, Y0_h = _np(ad0, Y0)
    worst, cases = 0.0, 0
    for n_ph in (1e3, 1e6):
        gain = est.photon_gain(n_ph)
        assert gain * Y0_h.max() <= 2.0 ** 31 - 10.0
        forms = [dict(gain=gain), dict(gain=gain, background=5.0), dict(gain=gain, read_noise=2.0, qe=0.8), dict(gain=gain, read_noise=3.0, background=5.0)]
        per = gain * np.linspace(0.5, 2.0, batch)
        forms.append(dict(gain=_dev(per), read_noise=1.5))
        for kw in forms:
            det = pkg.DetectorNoise(seed=SEED, first=11, **kw)
            for step in (0, 5):
                ad_f, Y_f = est.apply_device(s, noise=det, step=step, want_Y=True)
                ad_n = est.apply_device(s, noise=det, step=step)                                  # Y_out = NULL
                Y_c = pkg.detector_read(Y0, det, step=step)
                ad_f, Y_f, ad_n, Y_c = _np(ad_f, Y_f, ad_n, Y_c)
                assert np.all(np.isfinite(Y_f)) and np.all(np.isfinite(ad_f))
                assert np.array_equal(Y_f, Y_c), (kw, step, np.abs(Y_f - Y_c).max())
                assert np.array_equal(ad_n, ad_f)
                assert not np.array_equal(Y_f, Y0_h)                                              # (there is noise)
                err, bar = np.abs((ad_f - ad0_h) - (Y_f - Y0_h) @ G.T), _ad_bar(G, Y_f, Y0_h, b_s, p)
                worst = max(worst, np.max(err / bar))
                assert np.all(err <= bar), (kw, step, np.max(err / bar))
                cases += 1
        # without read-out noise and background the read-out is a whole number of photo-electrons
        cnt = _np(est.apply_device(s, noise=pkg.DetectorNoise(gain, seed=SEED), want_Y=True)[1]) * gain
        assert np.abs(cnt - np.round(cnt)).max() <= 1e-9 * max(1.0, cnt.max()) and cnt.min() >= 0.0
    print(f"2. {name}: Y_out fused == composed in {cases} cases; ad_est - ad_est0 against G (Y - Y0): worst {worst:.2e} of its bar")


# ---- 3. reduction to SIGMA --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["len64_d31", "len512_b1"])
def test_reduction_to_sigma_on_the_device(pkg, gpu, name):
    (est, D, A_s, b_s), scr = _estimator(pkg, name)
    batch = SHAPES[name][5]
    s = _dev(scr[:batch])
    sigma = est.snr_sigma(10.0)
    assert _np(est.apply_device(s, want_Y=True)[1]).max() <= 2.0 ** 31                            # (gain = 1: Y0 itself is lam)
    for step in (0, 5):
        ad_s, Y_s = est.apply_device(s, noise=pkg.EstimatorNoise(sigma=sigma, seed=SEED, first=11), step=step, want_Y=True)
        ad_d, Y_d = est.apply_device(s, noise=pkg.DetectorNoise(1.0, photon_noise=False, read_noise=sigma, seed=SEED, first=11), step=step, want_Y=True)
        ad_s, Y_s, ad_d, Y_d = _np(ad_s, Y_s, ad_d, Y_d)
        assert np.array_equal(Y_d, Y_s) and np.array_equal(ad_d, ad_s), (step, np.abs(Y_d - Y_s).max())
    print(f"3. {name}: photon_noise = 0, background = 0, qe = 1, gain = 1 == FMPC_NOISE_SIGMA, bit for bit")


# ---- 4. placement -----------------------------------------------------------------------------------------------------------
def test_a_realisation_gets_the_same_noise_wherever_it_sits(pkg, gpu):
    """len 64 (the general finish in either call): realisation R of a batch of 5 with first = 0 against the same screen alone with
    first = R, Y_out and ad_est bit for bit.  len 512: 21 screens take fmpc_est_finish_few<1>, 22 the general finish (the same PSF
    kernel) -- Y0 differs in its last bit between the two (|O|^2 is rounded in another order), the photo-electron count drawn
    from it does not, so Y_out is bit for bit and ad_est is held to the bar of test 2."""
    (est, D, A_s, b_s), scr = _estimator(pkg, "len64_d31")
    s5 = _dev(scr[:5])
    mk = lambda first, gain: pkg.DetectorNoise(gain, read_noise=2.0, background=1.0, seed=SEED, first=first)
    gain = est.photon_gain(1e4)
    ad5, Y5 = _np(*est.apply_device(s5, noise=mk(0, gain), step=2, want_Y=True))
    for R in (0, 3, 4):
        ad1, Y1 = _np(*est.apply_device(s5[R:R + 1], noise=mk(R, gain), step=2, want_Y=True))
        assert np.array_equal(Y1[0], Y5[R]) and np.array_equal(ad1[0], ad5[R]), R
    assert not np.array_equal(Y5[0], _np(est.apply_device(s5[:1], noise=mk(1, gain), step=2, want_Y=True)[1])[0])
    (est, D, A_s, b_s), scr = _estimator(pkg, "len512_b24")
    G = np.linalg.pinv(A_s.T @ A_s) @ A_s.T
    gain = est.photon_gain(1e4)
    s22 = _dev(scr[:22])
    ad_g, Y_g = _np(*est.apply_device(s22, noise=mk(0, gain), step=2, want_Y=True))              # 66 (screen, diversity) pairs: general
    ad_f, Y_f = _np(*est.apply_device(s22[:21], noise=mk(0, gain), step=2, want_Y=True))         # 63: few-screen finish
    Y0 = _np(est.apply_device(s22[:21], want_Y=True)[1])
    assert np.array_equal(Y_f, Y_g[:21]), np.abs(Y_f - Y_g[:21]).max()
    err, bar = np.abs(ad_f - ad_g[:21]), _ad_bar(G, Y_f, Y0, b_s, est.p)
    print(f"4. len 64: bit for bit; len 512 across the finish forms: Y_out bit for bit, ad_est {np.max(err / bar):.2e} of its bar")
    assert np.all(err <= bar)


# ---- 5. the counter on the device -------------------------------------------------------------------------------------------
def test_counter_on_the_device_under_a_graph(pkg, gpu):
    """One detector apply with `counter`, then counter.add_(1), captured as a single chain: three replays are three eager calls with
    step = 0, 1, 2, bit for bit, and differ from each other."""
    import gc
    import torch
    (est, D, A_s, b_s), scr = _estimator(pkg, "len64_d31")
    s = _dev(scr[:3]).transpose(-1, -2).contiguous()
    kw = dict(gain=est.photon_gain(1e4), read_noise=2.0, seed=SEED)
    eager = [_np(*est.apply_device(s, noise=pkg.DetectorNoise(**kw), step=k, want_Y=True, colmajor=True)) for k in range(3)]
    ctr = torch.zeros(1, dtype=torch.int64, device=gpu)
    det = pkg.DetectorNoise(counter=ctr, **kw)
    ad = torch.empty((3, est.nx), dtype=torch.float64, device=gpu)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g):
        _, Y = est.apply_device(s, noise=det, step=0, want_Y=True, colmajor=True, out=ad)
        ctr.add_(1)
    ctr.zero_()
    got = []
    for k in range(3):
        g.replay()
        got.append(_np(ad, Y))
        assert int(ctr.item()) == k + 1
    for k in range(3):
        for a, b in zip(got[k], eager[k]):
            assert np.array_equal(a, b), k
    assert not np.array_equal(got[0][1], got[1][1]) and not np.array_equal(got[1][0], got[2][0])
    print("5. three replays == eager steps 0, 1, 2")


# ---- 6. AOLoop --------------------------------------------------------------------------------------------------------------
def test_aoloop_with_detector_noise(pkg, gpu):
    """The small loop of test_aoloop_with_device_noise, (n, m, T) = (27, 144, 2) at len 64, batch 3, four steps with
    AOLoop.step(phase, noise=DetectorNoise(...)).  The form of check taken here: bit for bit against a second run of itself, and
    different from a run with another seed and from a noise-free run, at every step (the composed loop -- Y0 read through
    detector_read and handed back as Y - Y0 -- would need each step's screens before the step runs, which only the step builds).
    That `step` passes `steps_done` is seen against apply_device at that step on the loop's own screens."""
    from tests.util import handle_from_model
    R, steps, L = 3, 4, 64
    op = pkg.synthetic.estimator_optics(L)
    md = pkg.synthetic.make_model(27, 144, 2)
    rng = np.random.default_rng(4)
    a = np.stack([0.03 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    phase = _dev(np.tensordot(a, op["Z"][1:], axes=1) + 0.01 * rng.standard_normal((steps, R, L, L)))
    est = pkg.PhaseDiversityEstimator(op["pupil"], op["W"], op["zd_list"], op["dx"], op["range_min"] + 1, op["range_max"] + 1,
                                      op["A_s"], op["b_s"], AU=op["AU"])
    gain = est.photon_gain(1e4)

    def run(noise_of_step):
        h = handle_from_model(pkg, md)
        loop = pkg.AOLoop(h, est, op["Z"][1:], R, n_newton=1, k=1e-2)
        out = []
        for k in range(steps):
            nz = noise_of_step(k)
            u, adk = loop.step(phase[k], noise=nz)
            if nz is not None:                            # the step number the loop passed: the same call on the loop's own screens
                assert np.array_equal(_np(est.apply_device(loop.scrn, noise=nz, step=k, colmajor=True)), _np(adk))
            out.append(_np(u.clone(), adk.clone()))
        h.close()
        return out

    mk = lambda seed: pkg.DetectorNoise(gain, read_noise=2.0, seed=seed)
    fused, again, other, quiet = run(lambda k: mk(SEED)), run(lambda k: mk(SEED)), run(lambda k: mk(SEED + 1)), run(lambda k: None)
    for k in range(steps):
        for j in range(2):
            assert np.array_equal(fused[k][j], again[k][j]) and np.all(np.isfinite(fused[k][j])), (k, j)
        assert not np.array_equal(fused[k][1], other[k][1]) and not np.array_equal(fused[k][1], quiet[k][1])
    d = max(np.abs(fused[k][1] - quiet[k][1]).max() / np.abs(quiet[k][1]).max() for k in range(steps))
    print(f"6. AOLoop: repeats over {steps} steps; 1e4 photo-electrons per window move ad_est by {d:.2e} relative")
    est.close()
