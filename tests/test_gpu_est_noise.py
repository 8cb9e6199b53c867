"""GPU tests of the measurement noise drawn inside the estimator's finish pass (include/fastmpc.h: fmpc_noise,
fmpc_est_apply_noisy_device, fmpc_noise_normal_device).  Estimators are built as tests/test_gpu_estimator_shapes.py builds them
(its reference module, tests/estimator_shapes_ref.py); the draw's restatement is tests/noise_ref.py.  What is compared:
  1. the device fill against the host fill (1e-12 sigma: two libms on |g| <= 8.57), and with itself across batch splits (bits);
  2. SIGMA mode: the fused call against fill + fmpc_est_apply_device(noise = array), bit for bit, at every kernel form;
  3. SNR mode against the composition, bars from the test's own data: two fixed-order sums of p terms, eps = 2.2e-16;
  4. the realised SNR of one realisation; 5. independence of position in the batch; 6. the counter on the device under a graph;
  7. AOLoop.step with an EstimatorNoise against the same loop fed the composed tensors.
Every test prints the worst figure it saw."""
import ctypes as C

import numpy as np
import pytest

from tests import estimator_shapes_ref as sr
from tests import noise_ref as nr
from tests.util import rel_err
from tests.test_gpu_estimator_shapes import _build, _modes, FULL, TWO

pytestmark = pytest.mark.gpu

SEED = 20261019
EPS = 2.2e-16
# name: (len, zd_list, first, d, nx, batch) -- the kernel forms of fmpc_launch_estimator
SHAPES = {
    "len64_d31": (64, FULL, 17, 31, 27, 3),          # 4-wavefront PSF kernel, general finish
    "len64_d5_two": (64, TWO, 30, 5, 6, 3),          # two diversities, a small window, nx < one row block of the finish
    "len128_d32": (128, FULL, 0, 32, 27, 2),         # 8-wavefront PSF kernel, no padded column
    "len512_b1": (512, FULL, 241, 31, 27, 1),        # column split, fmpc_est_finish_few<2>
    "len512_b2": (512, FULL, 241, 31, 27, 2),
    "len512_b24": (512, FULL, 241, 31, 27, 24),      # general finish at nblk = 32
}
_EST, _SCR = {}, {}


def _estimator(pkg, name):
    """One handle per (len, zd, first, d, nx) for the module (len 512: a second to build), with its screens."""
    length, zd, first, d, nx, _ = SHAPES[name]
    key = (length, zd, first, d, nx)
    if key not in _EST:
        _EST[key] = _build(pkg, length, "disk", zd, first, d, nx, seed=length + d)
        _SCR[key] = sr.rough_screens(np.random.default_rng(length + d), _modes(pkg, length)[1:], 24 if length == 512 else 5)
    return _EST[key], _SCR[key]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _np(*ts):
    import torch
    torch.cuda.synchronize()
    out = tuple(t.cpu().numpy() for t in ts)
    return out if len(out) > 1 else out[0]


# ---- 1. the fill ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,p", [(3, 50), (4, 2883), (2, 51)])
def test_fill_device_against_host(pkg, gpu, batch, p):
    worst = 0.0
    for seed in (SEED, 0xF00DFACE12345678):
        for step in (0, 1, 2 ** 32 + 5):
            for first in (0, 7):
                for sigma in (1.0, 0.37):
                    nz = pkg.EstimatorNoise(sigma=sigma, seed=seed, first=first)
                    got = _np(pkg.normal_noise(batch, p, nz, step=step))
                    ref = pkg.normal_noise_host(batch, p, nz, step=step)
                    worst = max(worst, np.abs(got - ref).max() / sigma)
                    assert np.abs(got - ref).max() <= 1e-12 * sigma, (seed, step, first, sigma)
    print(f"1. fill ({batch}, {p}) device against host: worst {worst:.2e} sigma")
    # against the numpy restatement too, once
    assert np.abs(_np(pkg.normal_noise(batch, p, pkg.EstimatorNoise(sigma=1.0, seed=SEED), step=3)) - nr.fill(batch, p, SEED, 3)).max() <= 1e-12


def test_fill_is_bitwise_across_splits_strides_and_sigma_dev(pkg, gpu):
    import torch
    p = 2883
    one = _np(pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED), step=2))
    a = _np(pkg.normal_noise(2, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED), step=2))
    b = _np(pkg.normal_noise(3, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED, first=2), step=2))
    assert np.array_equal(one, np.concatenate([a, b]))
    # per-realisation sigma from the device: row r is sigma_r times the unit draw, one rounded product
    sig = np.array([0.5, 0.0, 2.0, 1e-3, 7.25])
    unit = _np(pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=1.0, seed=SEED), step=2))
    per = _np(pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=_dev(sig), seed=SEED), step=2))
    assert np.array_equal(per, sig[:, None] * unit) and np.array_equal(per[0], one[0])
    # ld > p: the padding stays; odd p: the last pair is half written
    out = torch.full((5, 2890), -7.0, dtype=torch.float64, device=gpu)
    pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED), step=2, out=out)
    o = _np(out)
    assert np.array_equal(o[:, :p], one) and np.all(o[:, p:] == -7.0)
    # the counter on the device is added to the step
    ctr = torch.tensor([2], dtype=torch.int64, device=gpu)
    assert np.array_equal(_np(pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED, counter=ctr), step=0)), one)
    assert np.array_equal(_np(pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED, counter=ctr), step=2 ** 64 - 2)),
                          _np(pkg.normal_noise(5, p, pkg.EstimatorNoise(sigma=0.5, seed=SEED), step=0)))      # (wraps like the 64-bit sum it is)


# ---- 2. SIGMA mode: fused against composed ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_sigma_mode_fused_equals_composed_bitwise(pkg, gpu, name):
    (est, D, A_s, b_s), scr = _estimator(pkg, name)
    batch = SHAPES[name][5]
    s = _dev(scr[:batch])
    sigma = est.snr_sigma(10.0)
    assert abs(sigma - np.sqrt(np.mean(b_s ** 2) * 0.1)) <= 2 * est.p * EPS * sigma               # (a sum of p squares in another order)
    cases = [("fixed", sigma, sigma)]
    if name in ("len64_d31", "len512_b2", "len512_b24"):
        per = sigma * np.linspace(0.25, 3.0, batch)
        cases.append(("sigma_dev", _dev(per), per))
    for what, sg, sg_host in cases:
        for step in (0, 5):
            nz = pkg.EstimatorNoise(sigma=sg, seed=SEED, first=11)
            fill = pkg.normal_noise(batch, est.p, nz, step=step)
            ad_c, Y_c = est.apply_device(s, noise=fill, want_Y=True)
            ad_f, Y_f, sig_f = est.apply_device(s, noise=nz, step=step, want_Y=True, want_sigma=True)
            ad_n = est.apply_device(s, noise=nz, step=step)                                       # Y_out = NULL, sigma_out = NULL
            ad_c, Y_c, ad_f, Y_f, sig_f, ad_n, fill_h = _np(ad_c, Y_c, ad_f, Y_f, sig_f, ad_n, fill)
            assert np.all(np.isfinite(Y_f)) and np.all(np.isfinite(ad_f))
            assert np.array_equal(Y_f, Y_c), (what, step, np.abs(Y_f - Y_c).max())
            assert np.array_equal(ad_f, ad_c) and np.array_equal(ad_n, ad_c), (what, step)
            assert np.array_equal(sig_f, np.broadcast_to(sg_host, (batch,)))
            assert np.abs(fill_h).max() > 0.0 and not np.array_equal(ad_f, _np(est.apply_device(s)))   # (there is noise)
    print(f"2. {name}: fused == composed, {len(cases)} sigma forms x 2 steps")


# ---- 3. SNR mode against the composition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("snr_db", [10.0, 30.0])
@pytest.mark.parametrize("name", ["len64_d31", "len64_d5_two", "len512_b1", "len512_b2"])
def test_snr_mode_against_the_composition(pkg, gpu, name, snr_db):
    (est, D, A_s, b_s), scr = _estimator(pkg, name)
    batch, p = SHAPES[name][5], est.p
    s = _dev(scr[:batch])
    _, Y0 = est.apply_device(s, want_Y=True)
    nz = pkg.EstimatorNoise(snr_db=snr_db, seed=SEED, first=3)
    ad, Y, sig = est.apply_device(s, noise=nz, step=4, want_Y=True, want_sigma=True)
    ad_n, sig_n = est.apply_device(s, noise=nz, step=4, want_sigma=True)                         # Y_out = NULL: no pass over Y
    g = pkg.normal_noise(batch, p, pkg.EstimatorNoise(sigma=1.0, seed=SEED, first=3), step=4)
    Y0, ad, Y, sig, ad_n, sig_n, g = _np(Y0, ad, Y, sig, ad_n, sig_n, g)
    assert np.array_equal(ad_n, ad) and np.array_equal(sig_n, sig)
    sig_ref = np.sqrt(np.mean(Y0 ** 2, axis=1) * 10.0 ** (-snr_db / 10.0))
    G = np.linalg.pinv(A_s.T @ A_s) @ A_s.T
    es = np.abs(sig - sig_ref) / sig_ref
    Yref = Y0 + sig_ref[:, None] * g
    ybar = 4 * p * EPS * (np.abs(Y0) + sig_ref[:, None] * np.abs(g))
    adref = (Yref - b_s) @ G.T
    adbar = 4 * p * EPS * ((np.abs(Y0 - b_s) + sig_ref[:, None] * np.abs(g)) @ np.abs(G).T)
    print(f"3. {name} snr {snr_db}: sigma {es.max():.2e} (bar {2 * p * EPS:.2e}), Y {np.max(np.abs(Y - Yref) / ybar):.2e} of its bar, "
          f"ad {np.max(np.abs(ad - adref) / adbar):.2e} of its bar")
    assert np.all(es <= 2 * p * EPS)
    assert np.all(np.abs(Y - Yref) <= ybar)
    assert np.all(np.abs(ad - adref) <= adbar)


# ---- 4. the realised SNR ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("snr_db", [10.0, 30.0])
def test_realised_snr(pkg, gpu, snr_db):
    """Over one realisation of p = 2883 the sample variance of the noise is within 4 standard errors, 4 sqrt(2 / p), of sigma^2 =
    mean(Y0^2) 10^(-snr / 10) (tests/test_host_noise_api.py checks that the draw at this seed stays inside that bound)."""
    (est, D, A_s, b_s), scr = _estimator(pkg, "len64_d31")
    p = est.p
    assert p == 2883
    s = _dev(scr[:3])
    _, Y0 = est.apply_device(s, want_Y=True)
    _, Y = est.apply_device(s, noise=pkg.EstimatorNoise(snr_db=snr_db, seed=SEED), step=1, want_Y=True)
    Y0, Y = _np(Y0, Y)
    for r in range(3):
        ratio = np.sum(Y0[r] ** 2) / np.sum((Y[r] - Y0[r]) ** 2)
        got_db = 10 * np.log10(ratio)
        print(f"4. realisation {r}: {got_db:.3f} dB for {snr_db} dB")
        assert abs(10.0 ** (snr_db / 10.0) / ratio - 1.0) <= 4 * np.sqrt(2.0 / p), (r, got_db)
        assert abs(got_db - snr_db) <= 0.24, (r, got_db)                                        # (the bar this feature was specified with; tighter than 4 s.e., which is 0.46 dB)


# ---- 5. independence of position ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sigma", "snr"])
@pytest.mark.parametrize("name", ["len64_d31", "len512_b1"])
def test_a_realisation_gets_the_same_noise_wherever_it_sits(pkg, gpu, name, mode):
    """Realisation R of a batch of 5 with first = 0 against the same screen alone with first = R.  len 64: the same kernel form,
    everything bit for bit.  len 512: 5 screens take the PSF kernel without the column split and fmpc_est_finish_few<1>, a lone
    screen the split and fmpc_est_finish_few<2> -- two summation orders of Y0, which differ (found: they do), so Y0 is held to the
    1e-11 of tests/test_gpu_estimator.py between two orders; the noise term itself is bit for bit: Y_M = Y0 + fill exactly, with
    the fill of either placement."""
    (est, D, A_s, b_s), scr = _estimator(pkg, name)
    s5 = _dev(scr[:5])
    mk = (lambda first: pkg.EstimatorNoise(sigma=est.snr_sigma(10.0), seed=SEED, first=first)) if mode == "sigma" else \
         (lambda first: pkg.EstimatorNoise(snr_db=10.0, seed=SEED, first=first))
    ad5, Y5, sg5 = _np(*est.apply_device(s5, noise=mk(0), step=2, want_Y=True, want_sigma=True))
    _, Y05 = est.apply_device(s5, want_Y=True)
    Y05 = _np(Y05)
    unit5 = _np(pkg.normal_noise(5, est.p, pkg.EstimatorNoise(sigma=1.0, seed=SEED), step=2))
    worst = 0.0
    for R in (0, 3, 4):
        ad1, Y1, sg1 = _np(*est.apply_device(s5[R:R + 1], noise=mk(R), step=2, want_Y=True, want_sigma=True))
        _, Y01 = est.apply_device(s5[R:R + 1], want_Y=True)
        Y01 = _np(Y01)
        unit1 = _np(pkg.normal_noise(1, est.p, pkg.EstimatorNoise(sigma=1.0, seed=SEED, first=R), step=2))
        assert np.array_equal(unit1[0], unit5[R])                                               # the draw: bit for bit, always
        assert np.array_equal(Y1[0], Y01[0] + sg1[0] * unit1[0]) and np.array_equal(Y5[R], Y05[R] + sg5[R] * unit5[R])
        if name == "len64_d31":
            assert np.array_equal(ad1[0], ad5[R]) and np.array_equal(Y1[0], Y5[R]) and sg1[0] == sg5[R], R
        else:
            e0, ey, ea = rel_err(Y01[0], Y05[R]), rel_err(Y1[0], Y5[R]), rel_err(ad1[0], ad5[R])
            worst = max(worst, e0, ey, ea)
            assert e0 <= 1e-11 and ey <= 1e-11 and ea <= 1e-11 and abs(sg1[0] - sg5[R]) <= 1e-11 * sg5[R], (R, e0, ey, ea)
    print(f"5. {name} {mode}: " + ("bit for bit" if name == "len64_d31" else f"noise term bit for bit, Y0 between two summation orders {worst:.2e}"))


# ---- 6. the counter on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sigma", "snr"])
def test_counter_on_the_device_under_a_graph(pkg, gpu, mode):
    """One noisy apply with `counter`, then counter.add_(1), captured as a single chain: three replays are three eager calls with
    step = 0, 1, 2, bit for bit, and differ from each other."""
    import gc
    import torch
    (est, D, A_s, b_s), scr = _estimator(pkg, "len64_d31")
    s = _dev(scr[:3]).transpose(-1, -2).contiguous()
    kw = dict(sigma=est.snr_sigma(10.0)) if mode == "sigma" else dict(snr_db=10.0)
    eager = [_np(*est.apply_device(s, noise=pkg.EstimatorNoise(seed=SEED, **kw), step=k, want_Y=True, want_sigma=True, colmajor=True)) for k in range(3)]
    ctr = torch.zeros(1, dtype=torch.int64, device=gpu)
    nz = pkg.EstimatorNoise(seed=SEED, counter=ctr, **kw)
    ad = torch.empty((3, est.nx), dtype=torch.float64, device=gpu)
    g = torch.cuda.CUDAGraph()
    gc.collect()
    with torch.cuda.graph(g):
        _, Y, sg = est.apply_device(s, noise=nz, step=0, want_Y=True, want_sigma=True, colmajor=True, out=ad)
        ctr.add_(1)
    ctr.zero_()
    got = []
    for k in range(3):
        g.replay()
        got.append(_np(ad, Y, sg))
        assert int(ctr.item()) == k + 1
    for k in range(3):
        for a, b in zip(got[k], eager[k]):
            assert np.array_equal(a, b), (mode, k)
    assert not np.array_equal(got[0][1], got[1][1]) and not np.array_equal(got[1][0], got[2][0])
    print(f"6. {mode}: three replays == eager steps 0, 1, 2")


# ---- 7. AOLoop ----------------------------------------------------------------------------------------------------------------
def test_aoloop_with_device_noise(pkg, gpu):
    """(n, m, T) = (27, 144, 2) at len 64, batch 3, three steps: AOLoop.step(phase, noise=EstimatorNoise(...)) against the same loop
    fed the composed tensors (the fill at step = steps_done), bit for bit in SIGMA mode at the sigma of 10 dB against the
    unaberrated image; a second loop with the same seed repeats it, another seed does not.  SNR mode (sigma_r from each step's own
    screens, which the fed-back loop only has once the step runs): repeats, is finite and differs from the noise-free loop."""
    import torch
    from tests.util import handle_from_model
    R, steps, L = 3, 3, 64
    op = pkg.synthetic.estimator_optics(L)
    md = pkg.synthetic.make_model(27, 144, 2)
    rng = np.random.default_rng(4)
    a = np.stack([0.03 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    phase = _dev(np.tensordot(a, op["Z"][1:], axes=1) + 0.01 * rng.standard_normal((steps, R, L, L)))
    est = pkg.PhaseDiversityEstimator(op["pupil"], op["W"], op["zd_list"], op["dx"], op["range_min"] + 1, op["range_max"] + 1,
                                      op["A_s"], op["b_s"], AU=op["AU"])
    sigma = est.snr_sigma(10.0)

    def run(noise_of_step):
        h = handle_from_model(pkg, md)
        loop = pkg.AOLoop(h, est, op["Z"][1:], R, n_newton=1, k=1e-2)
        out = []
        for k in range(steps):
            u, adk = loop.step(phase[k], noise=noise_of_step(k, loop))
            out.append(_np(u.clone(), adk.clone()))
        h.close()
        return out

    fused = run(lambda k, loop: pkg.EstimatorNoise(sigma=sigma, seed=SEED))
    composed = run(lambda k, loop: pkg.normal_noise(R, est.p, pkg.EstimatorNoise(sigma=sigma, seed=SEED), step=k))
    again = run(lambda k, loop: pkg.EstimatorNoise(sigma=sigma, seed=SEED))
    other = run(lambda k, loop: pkg.EstimatorNoise(sigma=sigma, seed=SEED + 1))
    quiet = run(lambda k, loop: None)
    snr = run(lambda k, loop: pkg.EstimatorNoise(snr_db=10.0, seed=SEED))
    snr_again = run(lambda k, loop: pkg.EstimatorNoise(snr_db=10.0, seed=SEED))
    for k in range(steps):
        for j in range(2):
            assert np.array_equal(fused[k][j], composed[k][j]) and np.array_equal(fused[k][j], again[k][j]), (k, j)
            assert np.array_equal(snr[k][j], snr_again[k][j]), (k, j)
            assert np.all(np.isfinite(snr[k][j]))
        assert not np.array_equal(fused[k][1], other[k][1]) and not np.array_equal(fused[k][1], quiet[k][1])
        assert not np.array_equal(snr[k][1], quiet[k][1])
    # (10 dB on these windows against screens of 0.03 rad: the noise dominates the estimate, as the figure shows)
    d = max(rel_err(fused[k][1], quiet[k][1]) for k in range(steps))
    print(f"7. AOLoop: fused == composed over {steps} steps; noise moves ad_est by {d:.2e} relative")
    est.close()
