"""AOLoop(sensor=sh): x0 of a step comes from the Shack-Hartmann sensor on the step's residual screen instead of the
phase-diversity estimator, and without the argument nothing changes.  A small handle (n = 9 modes, m = 16, T = 2) on a 64 x 64
grid, three steps, three realisations.  All equalities are of bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_loop_with_the_sensor(pkg, gpu):
    from tests.util import handle_from_model
    R, steps, L, n = 3, 3, 64, 9
    opt = pkg.reference_optics(L, N=3)                                                    # 10 modes: the piston and n = 9
    md = pkg.synthetic.make_model(n, 16, 2)
    rng = np.random.default_rng(9)
    a = np.stack([0.3 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    Zc = opt.Z[1:].contiguous()                                                           # [j, column, row]
    phase = torch.tensordot(torch.from_numpy(a).to(gpu), Zc, dims=1) + 0.01 * torch.from_numpy(rng.standard_normal((steps, R, L, L))).to(gpu)
    sen = pkg.ShackHartmann(pkg.reference_pupil(L), 16)
    runs = {}
    for which in ("plain", "none", "sensor", "noisy"):
        h = handle_from_model(pkg, md)
        est = opt.estimator(opt.Z, skip=1)
        if which == "plain":
            loop = pkg.AOLoop(h, est, Zc, R, n_newton=1, k=1e-2, z_colmajor=True)       # built without the argument
            assert loop.sensor is None
        elif which == "none":
            loop = pkg.AOLoop(h, est, Zc, R, n_newton=1, k=1e-2, z_colmajor=True, sensor=None)
        else:
            if which == "sensor":
                with pytest.raises(ValueError):                                           # not calibrated yet: no modes
                    pkg.AOLoop(h, est, Zc, R, z_colmajor=True, sensor=sen)
                sen.set_reference()
                D, sv, rank = sen.calibrate(Zc, colmajor=True)
                assert rank == n and sen.nmode == n and sv[0] / sv[-1] < 50
                with pytest.raises(ValueError):                                           # a sensor on another grid
                    pkg.AOLoop(h, est, Zc, R, z_colmajor=True, sensor=pkg.ShackHartmann(np.ones((128, 128)), 16))
            loop = pkg.AOLoop(h, est, Zc, R, n_newton=1, k=1e-2, z_colmajor=True, sensor=sen)
        det = pkg.DetectorNoise(gain=50.0, photon_noise=True, read_noise=1.0, seed=4) if which == "noisy" else None
        seen = []
        for s in range(steps):
            u, x0 = loop.step(phase[s], noise=det, colmajor=True)
            if which == "sensor":
                assert torch.equal(x0, sen.coefficients(loop.scrn, colmajor=True)), s
            if which == "noisy":
                fr = sen.measure(loop.scrn, want_frame=True, want_coef=False, want_slopes=False, colmajor=True)
                noisy = pkg.detector_read(fr.view(R, -1), det, step=s)
                sl, cf = sen.slopes_from_frame(noisy, want_coef=True)
                assert torch.equal(x0, cf) and not torch.equal(x0, sen.coefficients(loop.scrn, colmajor=True)), s
            seen.append(dict(u=u.clone(), x0=x0.clone()))
        if which == "sensor":
            with pytest.raises(TypeError):
                loop.step(phase[0], noise=pkg.EstimatorNoise(sigma=1.0), colmajor=True)
        torch.cuda.synchronize()
        runs[which] = seen
        est.close(); h.close()
    for s in range(steps):
        assert torch.equal(runs["plain"][s]["u"], runs["none"][s]["u"]) and torch.equal(runs["plain"][s]["x0"], runs["none"][s]["x0"]), s
        assert bool(torch.isfinite(runs["sensor"][s]["u"]).all()) and not torch.equal(runs["sensor"][s]["x0"], runs["plain"][s]["x0"])
    # the sensor's x0 of the first step is close to the coefficients that made the screen (0.01 rad of roughness on top)
    err = (runs["sensor"][0]["x0"] - torch.from_numpy(a[0]).to(gpu)).norm(dim=1) / torch.from_numpy(a[0]).to(gpu).norm(dim=1)
    print("sensor x0 against the generating coefficients:", err.tolist())
    assert bool((err < 0.1).all())
    sen.close(); opt.close()
