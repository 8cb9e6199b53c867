"""The science camera on the device (fmpc_sci_*, pkg.ScienceCamera) against the numpy restatement tests/science_ref.py.

Shapes are the smallest that reach each path: len 64 (a wavefront sees at most 2 k-steps), 128 and 192 (no power of two), every
window d, samplings 1, 2 and 2.5, batches 1, 3 and 67 -- both kernel forms, asserted through `last_form` -- and a pupil with an
obstruction off centre, amplitude in [0.5, 1.5], an empty row block and empty leading columns.

Bars.  Image: 1e-10 of a screen's norm, the bar tests/test_gpu_estimator.py sets for the same arithmetic.  MEAN and RMS: 1e-11 of
sigma against long double, also at mu = 1e4 sigma, where the one-pass formula sum a phi^2 - (sum a phi)^2 / sum a is 4e-9 off and
the merged triples 1e-14 (CPU, numpy).  STREHL and MARECHAL: 1e-12 relative.  MIN and MAX: equal.  Everything that is called an
equality is one of bits."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import science_ref as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "model_approx_As_bs.npz")
DX, AU = 0.5, 3.0
SCALE = DX ** 4 * AU


@functools.lru_cache(maxsize=None)
def pupil_of(length):
    A = sr.make_pupil(length)
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def screens_of(length, batch):
    s = sr.make_screens(length, batch, np.random.default_rng(100 * length + batch))
    s.setflags(write=False)
    return s


def dev(a, gpu):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to(gpu)


def camera(pkg, length, d, s):
    return pkg.ScienceCamera(pupil_of(length), d=d, sampling=s, dx=DX, AU=AU)


def expected_form(pkg, length, count):
    return pkg.FMPC_SCI_FORM_FEW if count * (length // 16) <= 256 else pkg.FMPC_SCI_FORM_STANDARD


def check_quality(got, A, phi, tag):
    want = sr.quality(A, phi)
    sig = float(want[sr.RMS])
    e_mu, e_sig = abs(float(got[sr.MEAN] - want[sr.MEAN])) / sig, abs(float(got[sr.RMS] - want[sr.RMS])) / sig
    e_s = abs(float(got[sr.STREHL] - want[sr.STREHL])) / float(want[sr.STREHL])
    e_m = abs(float(got[sr.MARECHAL] - want[sr.MARECHAL])) / float(want[sr.MARECHAL])
    print(tag, "mean %.2e rms %.2e (of sigma) strehl %.2e marechal %.2e" % (e_mu, e_sig, e_s, e_m))
    assert e_mu <= 1e-11 and e_sig <= 1e-11, (tag, e_mu, e_sig)
    assert e_s <= 1e-12 and e_m <= 1e-12, (tag, e_s, e_m)
    assert got[sr.MIN] == float(want[sr.MIN]) and got[sr.MAX] == float(want[sr.MAX]), tag


CASES = [(64, 16, 1.0, 67), (64, 64, 2.5, 67), (64, 32, 2.0, 1), (64, 48, 1.0, 3), (128, 32, 1.0, 67), (128, 48, 2.5, 3), (128, 64, 2.0, 1),
         (192, 64, 2.0, 3), (192, 16, 2.5, 1), (192, 32, 1.0, 3)]


@pytest.mark.parametrize("length,d,s,batch", CASES)
def test_image_and_quality_against_numpy(pkg, gpu, length, d, s, batch):
    A, phi = pupil_of(length), screens_of(length, batch)
    cam = camera(pkg, length, d, s)
    assert (cam.len, cam.d, cam.sampling) == (length, d, s)
    ra, ra2, rI0 = sr.sums(A, SCALE)
    assert abs(cam.sum_a - ra) <= 1e-15 * ra and abs(cam.sum_a2 - ra2) <= 1e-15 * ra2 and abs(cam.I0 - rI0) <= 1e-15 * rI0
    img, q = cam.expose(dev(phi, gpu))
    assert cam.last_form == expected_form(pkg, length, batch)
    img, q = img.cpu().numpy(), q.cpu().numpy()
    assert img.shape == (batch, d, d) and q.shape == (batch, pkg.FMPC_SCI_FIELDS)
    check = range(batch) if length == 64 else range(min(batch, 3))            # (the long-double reference of 67 large screens is slow)
    worst = 0.0
    for b in check:
        want = sr.colmajor(sr.image_dft(A, phi[b], d, s, SCALE))
        err = np.linalg.norm(img[b] - want) / np.linalg.norm(want)
        worst = max(worst, err)
        assert err <= 1e-10, (b, err)
        check_quality(q[b], A, phi[b], "screen %d" % b)
        c = img[b, d // 2, d // 2] / cam.I0
        assert abs(c - q[b, sr.STREHL]) <= 1e-12 * c, (b, c, q[b, sr.STREHL])
    print("image", (length, d, s, batch), "worst rel_err %.2e" % worst)
    if s == int(s) and length == 64:                                           # the FFT form, for whoever distrusts the long-double one
        want = sr.colmajor(sr.image_fft(A, phi[0], d, s, SCALE))
        assert np.linalg.norm(img[0] - want) <= 1e-10 * np.linalg.norm(want)
    cam.close()


def test_reference_pin(pkg, gpu):
    """reference_science_camera(32, 1) with one zero screen at len 512 is the zero-diversity block of the reference's b_s."""
    cam = pkg.reference_science_camera(32, 1.0)
    img, q = cam.expose(torch.zeros((512, 512), dtype=torch.float64, device=gpu))
    assert cam.last_form == pkg.FMPC_SCI_FORM_FEW
    img = img.cpu().numpy()[0].T                                               # [u, v]
    b = np.load(FIX)["b_s"].reshape(-1)[961:1922].reshape(31, 31, order="F")
    err = np.linalg.norm(img[1:, 1:] - b) / np.linalg.norm(b)
    print("b_s block %.2e  I0 %.2e" % (err, abs(cam.I0 - img[16, 16]) / cam.I0))
    assert err <= 1e-12, err
    assert abs(cam.I0 - img[16, 16]) <= 1e-13 * cam.I0
    q = q.cpu().numpy()[0]
    assert q[sr.MEAN] == 0 and q[sr.RMS] == 0 and abs(q[sr.STREHL] - 1) <= 1e-13 and q[sr.MARECHAL] == 1 and q[sr.MIN] == 0 and q[sr.MAX] == 0
    opt = pkg.reference_optics(64)                                             # the helper the pupil moved to gives what it gave
    assert np.array_equal(opt.pupil, pkg.reference_pupil(64, 6.5e-6))
    opt.close(); cam.close()


@pytest.mark.parametrize("length", [64, 128])
def test_quality_of_a_large_mean_and_of_small_noise(pkg, gpu, length):
    A = pupil_of(length)
    rng = np.random.default_rng(length)
    big = 3000.0 + 0.3 * rng.standard_normal((length, length))               # mu = 1e4 sigma
    small = 0.01 * rng.standard_normal((length, length))
    cam = camera(pkg, length, 16, 1.0)
    q = cam.quality(dev(np.stack([big, small]), gpu)).cpu().numpy()
    check_quality(q[0], A, big, "mu = 1e4 sigma")
    check_quality(q[1], A, small, "sigma = 0.01")
    assert abs((1 - q[1, sr.STREHL]) / q[1, sr.RMS] ** 2 - 1) <= 1e-3
    cam.close()


def test_bits_do_not_depend_on_batch_place_workspace_or_what_is_asked(pkg, gpu):
    length, d, s = 64, 48, 2.5
    cam = camera(pkg, length, d, s)
    phi = dev(screens_of(length, 67), gpu)
    img, q = cam.expose(phi)
    assert cam.last_form == pkg.FMPC_SCI_FORM_STANDARD
    one_i, one_q = cam.expose(phi[41])                                         # alone: the few-screens form
    assert cam.last_form == pkg.FMPC_SCI_FORM_FEW
    assert torch.equal(one_i[0], img[41]) and torch.equal(one_q[0], q[41])
    small = torch.empty(cam.workspace_bytes(1), dtype=torch.uint8, device=gpu)
    big = torch.empty(3 * cam.workspace_bytes(67) + 8, dtype=torch.uint8, device=gpu)
    assert 0 < cam.workspace_bytes(1) <= cam.workspace_bytes(3) <= cam.workspace_bytes(67) <= cam.workspace_bytes(2000) <= cam.workspace_bytes(100000)
    assert cam.workspace_bytes(0) == cam.workspace_bytes(1) and cam.workspace_bytes(-1) == 0
    for ws in (small, big):
        i2, q2 = cam.expose(phi, workspace=ws)
        assert torch.equal(i2, img) and torch.equal(q2, q)
    assert torch.equal(cam.quality(phi), q)                                    # no matrix instruction, the same rows
    only_i, none_q = cam.expose(phi, want_quality=False)
    assert none_q is None and torch.equal(only_i, img)
    # row-major screens are transposed on the way in
    i3, q3 = cam.expose(phi.transpose(-1, -2).contiguous(), colmajor=True)
    assert torch.equal(i3, img) and torch.equal(q3, q)
    # accumulate
    a, _ = cam.expose(phi[:3], want_quality=False)
    b, _ = cam.expose(phi[3:6], want_quality=False)
    acc = a.clone()
    out_i, _ = cam.expose(phi[3:6], image=acc, accumulate=True, want_quality=False)
    assert out_i is acc and torch.equal(acc, a + b)
    # padded quality rows
    pad = torch.full((67, 9), -7.0, dtype=torch.float64, device=gpu)
    cam.expose(phi, want_image=False, quality=pad)
    assert torch.equal(pad[:, :6], q) and bool((pad[:, 6:] == -7.0).all())
    cam.close()


def test_non_finite_pixels(pkg, gpu):
    length, d = 64, 32
    A = pupil_of(length)
    cam = camera(pkg, length, d, 2.0)
    base = screens_of(length, 3)
    img0, q0 = cam.expose(dev(base, gpu))
    inside = tuple(np.argwhere(A != 0)[37])
    outside = (int(length * 0.56 + 0.038 * length), int(length * 0.58 - 0.057 * length))      # in the obstruction: columns the kernel visits
    assert A[outside] == 0 and A[outside[0], :outside[1]].any() and A[outside[0], outside[1]:].any()
    for bad in (float("nan"), float("inf"), 2.0e6, -2.0e6):
        phi = base.copy(); phi[1][inside] = bad
        img, q = cam.expose(dev(phi, gpu))
        assert bool(torch.isnan(img[1]).all()) and bool(torch.isnan(q[1]).all()), bad
        assert torch.equal(img[0], img0[0]) and torch.equal(img[2], img0[2]) and torch.equal(q[0], q0[0]) and torch.equal(q[2], q0[2]), bad
        only, _ = cam.expose(dev(phi, gpu), want_quality=False)
        assert bool(torch.isnan(only[1]).all()) and torch.equal(only[0], img0[0])
        phi = base.copy(); phi[1][outside] = bad                                # where A = 0 nothing is read into any arithmetic
        phi[1][0, :] = bad; phi[1][:, 0] = bad
        img, q = cam.expose(dev(phi, gpu))
        assert torch.equal(img, img0) and torch.equal(q, q0), bad
    cam.close()


def test_summary(pkg, gpu):
    length, d, s = 64, 64, 1.0                                                  # the window is the whole DFT plane
    A = pupil_of(length)
    cam = camera(pkg, length, d, s)
    phi = screens_of(length, 9).reshape(3, 3, length, length)                   # three frames of three realisations
    acc = torch.zeros((3, d, d), dtype=torch.float64, device=gpu)
    strehl = []
    for f in range(3):
        _, q = cam.expose(dev(phi[f], gpu), image=acc, accumulate=True)
        strehl.append(q[:, sr.STREHL].cpu().numpy())
    out = cam.summary(acc, frames=3).cpu().numpy()
    assert out.shape == (3, 2 + d // 2)
    imgs = acc.cpu().numpy()
    for r in range(3):
        assert abs(out[r, 1] - 1) <= 1e-13, out[r, 1]                           # Parseval
        assert abs(out[r, 0] - np.mean([st[r] for st in strehl])) <= 1e-12 * out[r, 0]
        want = sr.summary(imgs[r].T, 3, d // 2, A, s, SCALE)
        assert np.abs(out[r] - want).max() <= 1e-12, np.abs(out[r] - want).max()
        assert np.all(np.diff(out[r, 2:]) >= 0)
    short = cam.summary(acc, frames=3, nrad=5).cpu().numpy()
    assert short.shape == (3, 7) and np.array_equal(short, out[:, :7])
    # another window and sampling: against the reference alone
    cam2 = camera(pkg, 128, 48, 2.5)
    img, _ = cam2.expose(dev(screens_of(128, 3), gpu))
    out2 = cam2.summary(img, frames=1).cpu().numpy()
    for r in range(3):
        want = sr.summary(img[r].cpu().numpy().T, 1, 24, pupil_of(128), 2.5, SCALE)
        assert np.abs(out2[r] - want).max() <= 1e-12 and 0 < out2[r, 1] < 1
    cam.close(); cam2.close()


def test_expose_records_into_a_graph(pkg, gpu):
    length, d = 64, 32
    cam = camera(pkg, length, d, 2.0)
    phi = dev(screens_of(length, 3), gpu)
    ws = torch.empty(cam.workspace_bytes(3), dtype=torch.uint8, device=gpu)
    acc = torch.zeros((3, d, d), dtype=torch.float64, device=gpu)
    q = torch.zeros((3, pkg.FMPC_SCI_FIELDS), dtype=torch.float64, device=gpu)
    run = lambda: cam.expose(phi, image=acc, accumulate=True, quality=q, colmajor=True, workspace=ws)
    for _ in range(3):
        run()                                                                   # eager, also the warm-up
    torch.cuda.synchronize()
    eager, eager_q = acc.clone(), q.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    acc.zero_(); q.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(acc, eager) and torch.equal(q, eager_q)
    cam.close()


def test_argument_errors_with_a_camera(pkg, gpu):
    lib = pkg.load()
    cam = camera(pkg, 64, 16, 1.0)
    E_NULL, E_DIM = pkg.FMPC_E_NULL, pkg.FMPC_E_DIM
    phi = dev(screens_of(64, 3), gpu)
    img = torch.zeros((3, 16, 16), dtype=torch.float64, device=gpu); q = torch.zeros((3, 6), dtype=torch.float64, device=gpu)
    ws = torch.empty(cam.workspace_bytes(3), dtype=torch.uint8, device=gpu)
    vp = lambda t: C.c_void_p(t.data_ptr())
    call = lambda batch=3, s=vp(phi), i=vp(img), acc=0, qq=vp(q), ldq=6, w=vp(ws), wb=ws.numel(): lib.fmpc_sci_expose_device(cam._h, batch, s, i, acc, qq, ldq, w, wb, None)
    assert call(s=None) == E_NULL and call(i=None, qq=None) == E_NULL and call(w=None) == E_NULL
    assert call(s=None, batch=-1) == E_NULL                                    # pointers before sizes
    assert call(batch=-1) == E_DIM and call(acc=2) == E_DIM and call(ldq=5) == E_DIM and call(ldq=-1) == E_DIM
    assert call(wb=cam.workspace_bytes(1) - 8) == E_DIM and call(w=C.c_void_p(ws.data_ptr() + 4)) == E_DIM
    assert call(batch=0) == 0 and call(ldq=0) == 0 and call() == 0
    out = torch.zeros((3, 10), dtype=torch.float64, device=gpu)
    summ = lambda batch=3, i=vp(img), frames=1, nrad=8, o=vp(out): lib.fmpc_sci_summary_device(cam._h, batch, i, frames, nrad, o, None)
    assert summ(i=None) == E_NULL and summ(o=None) == E_NULL
    assert summ(batch=-1) == E_DIM and summ(frames=0) == E_DIM and summ(nrad=9) == E_DIM and summ(nrad=-1) == E_DIM
    assert summ(batch=0) == 0 and summ(nrad=0) == 0 and summ() == 0
    ln, d, s = C.c_int(), C.c_int(), C.c_double()
    assert lib.fmpc_sci_dims(cam._h, C.byref(ln), C.byref(d), C.byref(s), None, None, None) == 0 and (ln.value, d.value, s.value) == (64, 16, 1.0)
    torch.cuda.synchronize()
    cam.close()
