"""AOLoop(science=cam): the camera sees the residual screen of every step and changes nothing else.  At the README geometry on a
64 x 64 grid, three steps, three realisations, with the modal residual and with the mirror's zonal surface (dm=): u and ad_est
bit-identical to the loop without the camera, `science_quality` the camera's own rows of each step's `scrn`, `science_image` the
single exposures added in call order, `science_reset()` after the first step leaves two frames.  All equalities are of bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_dm", [False, True])
def test_loop_with_the_camera(pkg, gpu, with_dm):
    from tests.util import handle_from_model
    R, steps, L, d = 3, 3, 64, 32
    opt = pkg.reference_optics(L)
    md = pkg.synthetic.make_model(27, 144, 10)
    rng = np.random.default_rng(9)
    a = np.stack([0.03 * pkg.synthetic.make_realisation(md, r=r, steps=steps)[1:steps + 1] for r in range(R)], axis=1)
    Zc = opt.Z[1:].contiguous()                                                           # [j, column, row]
    phase = torch.tensordot(torch.from_numpy(a).to(gpu), Zc, dims=1) + 0.01 * torch.from_numpy(rng.standard_normal((steps, R, L, L))).to(gpu)
    cam = pkg.reference_science_camera(d=d, sampling=2.0, length=L)
    kw = dict(dm=pkg.reference_dm(L, 6.5e-6 * 512 / L)) if with_dm else {}
    runs = {}
    for which in ("plain", "science", "reset"):
        h = handle_from_model(pkg, md)
        est = opt.estimator(opt.Z, skip=1)
        if which == "plain":
            loop = pkg.AOLoop(h, est, Zc, R, n_newton=1, k=1e-2, z_colmajor=True, **kw)
            assert loop.science is None and not hasattr(loop, "science_image")
            with pytest.raises(ValueError):
                loop.science_reset()
        else:
            with pytest.raises(ValueError):                                               # a camera on another grid
                pkg.AOLoop(h, est, Zc, R, z_colmajor=True, science=pkg.reference_science_camera(d=16, length=128), **kw)
            loop = pkg.AOLoop(h, est, Zc, R, n_newton=1, k=1e-2, z_colmajor=True, science=cam, **kw)
            with pytest.raises(ValueError):
                loop.science_summary()                                                    # no frame yet
        seen = []
        for s in range(steps):
            u, x0 = loop.step(phase[s], colmajor=True)
            rec = dict(u=u.clone(), x0=x0.clone())
            if which != "plain":
                img, q = cam.expose(loop.scrn, colmajor=True)
                assert torch.equal(loop.science_quality, q) and torch.equal(loop.science_quality, cam.quality(loop.scrn, colmajor=True)), s
                rec.update(img=img, q=q)
                if which == "reset" and s == 0:
                    loop.science_reset()
                    assert loop.science_frames == 0 and not bool(loop.science_image.any())
            seen.append(rec)
        if which == "science":
            assert loop.science_frames == 3
            assert torch.equal(loop.science_image, (seen[0]["img"] + seen[1]["img"]) + seen[2]["img"])
            out = loop.science_summary()
            assert torch.equal(out, cam.summary(loop.science_image, 3)) and out.shape == (R, 2 + d // 2)
            # the long-exposure Strehl ratio is the mean of the frames'
            mean_s = (seen[0]["q"][:, pkg.FMPC_SCI_STREHL] + seen[1]["q"][:, pkg.FMPC_SCI_STREHL] + seen[2]["q"][:, pkg.FMPC_SCI_STREHL]) / 3
            assert bool(((out[:, 0] - mean_s).abs() <= 1e-12 * mean_s).all())
        if which == "reset":
            assert loop.science_frames == 2 and torch.equal(loop.science_image, seen[1]["img"] + seen[2]["img"])
            assert loop.science_summary(nrad=4).shape == (R, 6)
        torch.cuda.synchronize()
        runs[which] = seen
        est.close(); h.close()
    for s in range(steps):
        for other in ("science", "reset"):
            assert torch.equal(runs["plain"][s]["u"], runs[other][s]["u"]) and torch.equal(runs["plain"][s]["x0"], runs[other][s]["x0"]), (other, s)
    # the rows are measurements of real screens
    q0, q2 = runs["science"][0]["q"], runs["science"][2]["q"]
    assert bool((q0[:, pkg.FMPC_SCI_RMS] > 0).all()) and bool(torch.isfinite(q2).all())
    cam.close(); opt.close()
