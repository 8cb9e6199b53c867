"""The atmosphere's kernels at the sizes where they take the paths that the reference's sizes (npix 128 and 512) take and
tests/test_gpu_atm.py does not reach: more than twelve row tiles of a line (a second and a third pass of a wavefront over the
operands), screens wider than one chunk of 64 columns and taller than one row per strip of the mean, sixteen layers, masks of
no and of one pixel, counters beyond 2^32, a recorded graph, `series`, and frozen flow on the output (tests/atm_flow.py).  The
yardsticks and helpers are those of tests/test_gpu_atm.py."""
import numpy as np
import pytest

from tests import atm_flow as af
from tests import atm_ref as ar
from tests.test_gpu_atm import _dev_state, _disk, _pair, one_extrusion, screens_against_the_restatement

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------- 1: more than twelve row tiles
# NT = ceil(W / 16) tiles of 16 rows, dealt to four wavefronts, three tiles of a wavefront per pass: 13 (pass 1 with one wavefront,
# its tile with one valid row), 14 (W % 4 = 1, the line at distance 208 is gathered across the ring's seam), 16 (W % 16 = 0,
# pass 1 with all four wavefronts), 25 (three passes).  Both axes and both directions in every case.
TILES = [
    (193, [1, 2], [(1.0, -1.0), (-1.0, 1.0)], [0.6, 0.4], 17, 0, False),
    (209, [1, 2, 208], [(1.0, 1.0), (-1.0, -1.0)], [0.6, 0.4], 3, 0, False),
    (256, [1, 2, 255], [(-1.0, 1.0), (0.5, -1.0)], [0.6, 0.4], 3, 1, False),
    (400, [1, 2], [(1.0, -1.0), (-1.0, 1.0)], [0.6, 0.4], 3, 0, True),
]


@pytest.mark.parametrize("W,stencil,winds,frac,batch,k0,random", TILES)
def test_one_extrusion_per_axis_beyond_twelve_tiles(pkg, gpu, W, stencil, winds, frac, batch, k0, random):
    """test_one_extrusion_per_axis_against_long_double at NT = 13, 14, 16 and 25.  At W = 400 the windows are N(0, 1) samples, not
    a start-up: the bound is a bound on one line given its operands, wherever the windows came from.
    Measured on one MI355X, the worst error of a new sample over its bound: 0.019, 0.013, 0.010, 0.008 at W = 193, 209, 256, 400
    (0.018 to 0.048 at W = 18 and 33 in tests/test_gpu_atm.py): the bound grows with W, the error of a sum with its root."""
    atm, ref = _pair(pkg, W, stencil, winds, frac, batch)
    if random:
        st = dict(windows=np.random.default_rng(W).standard_normal((len(winds), batch, W, W)), k=k0, counts=[W] * len(winds))
    else:                                                    # (a start-up in float64: seconds less than in long double, and a state all the same)
        st = ar.AtmRef(W, ref.s, ref.ext, frac, ref.vpx, ref.vpy, batch, ref.xi, dtype=np.float64).reset().state()
        st["k"] = k0
    one_extrusion(atm, ref, st)
    atm.close()


# ------------------------------------------------------------------------------------------- 2: chunks of columns, rows of a strip
def _moved(winds, steps, W):
    """Every ring origin and every fraction of every layer is non-zero after `steps` steps."""
    return all(n % W != 0 and f != 0.0 for vx, vy in winds for n, f in (ar.displacement(steps, vx), ar.displacement(steps, vy)))


WIDE = {
    18: ([1, 2], [(0.3, -2.6), (-1.3, 0.7)], [0.6, 0.4], 4),
    33: (None, [(2.6, 1.3), (-0.7, -1.9), (-2.6, 0.3)], [0.028, 0.004, 0.008], 4),
}


@pytest.mark.parametrize("out_len", [65, 100, 130, 200])
@pytest.mark.parametrize("W,batch", [(18, 17), (18, 40), (33, 17), (33, 40)])
def test_output_wider_than_a_chunk_and_taller_than_a_strip(pkg, gpu, W, batch, out_len):
    """test_output_against_the_restatement, same bound, at out_len 65 (a second chunk of one column, a strip of two rows), 100,
    130 (three chunks, the last of two columns) and 200 (four rows per strip), without a mask and with a disk."""
    stencil, winds, frac, steps = WIDE[W]
    assert _moved(winds, steps, W)
    atm, ref = _pair(pkg, W, stencil, winds, frac, batch)
    atm.reset().advance(steps)
    ref.load_state(_dev_state(atm))
    worst = screens_against_the_restatement(atm, ref, (out_len,))
    print(f"atm W={W} batch={batch} out_len={out_len}: worst error / bound {worst:.3f}")
    atm.close()


# sixteen layers, the most: distinct winds of m / 8 pixels (times 1.01, so that no displacement sits on an integer), layers
# that stand still on one axis or on both, one layer of fraction 0 (its new lines are A z alone)
L16_WINDS = [(0.0, 0.0) if l == 12 else (1.01 * (l - 8) / 8.0, 1.01 * ((5 * l) % 17 - 8) / 8.0) for l in range(16)]
L16_FRAC = [0.0 if l == 3 else 0.02 + 0.01 * l for l in range(16)]


def test_sixteen_layers_one_extrusion(pkg, gpu):
    """From k = 7 to 8 every moving axis of every layer extrudes exactly one line."""
    assert len(set(L16_WINDS)) == 16 and sum(vx == 0 for vx, _ in L16_WINDS) == 2 and sum(vy == 0 for _, vy in L16_WINDS) == 2
    atm, ref = _pair(pkg, 18, [1, 2], L16_WINDS, L16_FRAC, 17)
    ref.reset()
    st = ref.state()
    st["k"] = 7
    assert not st["windows"][3].any()                        # a start-up with fraction 0 is a window of zeros: give it another's,
    st["windows"][3] = st["windows"][4][::-1]                # so that its new lines A z are numbers with a bound above 0
    got = one_extrusion(atm, ref, st)
    moving = [int(vx != 0) + int(vy != 0) for vx, vy in L16_WINDS]
    assert got["counts"] == [18 + m for m in moving]
    atm.close()


def test_sixteen_layers_output(pkg, gpu):
    atm, ref = _pair(pkg, 18, [1, 2], L16_WINDS, L16_FRAC, 17)
    atm.reset().advance(2)
    st = _dev_state(atm)
    st["windows"][3] = st["windows"][4][::-1]                # (the layer of fraction 0 would add zeros: see above)
    atm.load_state(st).advance(3)
    ref.load_state(_dev_state(atm))
    assert all(w.any() for w in ref.win)
    worst = screens_against_the_restatement(atm, ref, (65,))
    print(f"atm 16 layers out_len=65: worst error / bound {worst:.3f}")
    atm.close()


def test_masks_of_no_pixel_of_one_pixel_and_of_every_pixel(pkg, gpu):
    """An empty mask: mu = 0 and the output is 0 everywhere, exactly.  A mask of one pixel: the mean of one value is that value, so
    the output is 0 there too, exactly -- the pixel sits in the third chunk of columns and in the second row of its strip.  A mask of
    ones at out_len 130 stays within the bound."""
    import torch
    stencil, winds, frac, steps = WIDE[18]
    atm, ref = _pair(pkg, 18, stencil, winds, frac, 17)
    atm.reset().advance(steps)
    ref.load_state(_dev_state(atm))
    n = 130
    none, one = np.zeros((n, n)), np.zeros((n, n))
    one[70, 129] = 1.0
    for mask in (none, one):
        out = torch.full((17, n, n), 7.0, dtype=torch.float64, device=gpu)
        atm.screen(n, mask=mask, out=out)
        torch.cuda.synchronize()
        assert bool((out == 0.0).all())
    plain = atm.screen(n).cpu().numpy()
    assert np.abs(plain[:, 70, 129]).min() > 0                # (the value whose mean is taken is not itself 0)
    screens_against_the_restatement(atm, ref, (n,), masks=(none, one, np.ones((n, n))))
    atm.close()


# ------------------------------------------------------------------------------------------- 3: frozen flow
def _device_provider(pkg):
    import torch

    def make(wind):
        speed, direction = af.speed_direction(*wind)
        atm = pkg.Atmosphere(af.R0, af.L0, [1.0], [speed], [direction], af.W - 1, float(af.W - 2), 1.0, af.BATCH, af.SEED, stencil=af.STENCIL)
        assert atm.pitch == 1.0
        atm.reset()

        def screens(k):
            atm.advance(k - atm.k)
            out = atm.screen(af.W - 1)
            torch.cuda.synchronize()
            return out.cpu().numpy()
        return screens, af.formed(speed, direction)
    return make


def test_frozen_flow_on_the_output(pkg, gpu):
    """include/fastmpc.h: "the content moves with the wind".  Seven winds, the screens four steps apart after 2 W + 3 steps; the
    winds whose pixel steps the library forms exactly are compared bit for bit (those along x at the least), the others within
    the bound derived in tests/atm_flow.py."""
    exact = af.frozen_flow(_device_provider(pkg))
    print("frozen flow, compared bit for bit:", exact)


def test_half_a_pixel_is_the_mean_of_two_neighbours(pkg, gpu):
    af.half_pixel(_device_provider(pkg))


# ------------------------------------------------------------------------------------------- 4: counters and indices at their limits
def test_extrusion_counts_beyond_32_bits(pkg, gpu):
    """step = (l << 48) | e with e = 2^32 - 1, 2^32 (layer 0) and 2^33 + 5, 2^33 + 6 (layer 1): the upper word of e reaches the draw
    on the device as it does on the host."""
    W, winds = 18, [(1.0, -1.0), (-1.0, 1.0)]
    atm, ref = _pair(pkg, W, [1, 2], winds, [0.6, 0.4], 17)
    xi = ar.xi_lib(pkg, 11, 17, W)
    assert not np.array_equal(xi(0, 2 ** 32), xi(0, 0)) and not np.array_equal(xi(1, 2 ** 33 + 5), xi(1, 5))
    assert not np.array_equal(xi(0, 2 ** 32), xi(1, 0))      # (1 << 32 in e is not 1 << 48 in step)
    ref.reset()
    st = ref.state()
    st["counts"] = [2 ** 32 - 1, 2 ** 33 + 5]
    got = one_extrusion(atm, ref, st)
    assert got["counts"] == [2 ** 32 + 1, 2 ** 33 + 7]
    atm.close()


def test_the_last_global_index(pkg, gpu):
    """first + batch = 2^32: the realisation with the global index 2^32 - 1, last of 17 and alone."""
    import torch
    W, winds, frac = 33, [(2.6, 1.0), (-0.3, -1.0), (-2.6, 0.3)], [0.028, 0.004, 0.008]
    mask = _disk(20)

    def run(batch, first):
        atm, _ = _pair(pkg, W, None, winds, frac, batch, first=first, ref=False)
        atm.reset()
        out = [atm.step(20, mask=mask).clone() for _ in range(3)]
        torch.cuda.synchronize()
        atm.close()
        return torch.stack(out).cpu().numpy()

    a, b = run(17, 2 ** 32 - 17), run(1, 2 ** 32 - 1)
    assert np.array_equal(a[:, 16], b[:, 0]) and np.abs(b).max() > 0
    assert not np.array_equal(a[:, 15], a[:, 16])
    with pytest.raises(pkg.FastMPCError) as e:
        _pair(pkg, W, None, winds, frac, 17, first=2 ** 32 - 16, ref=False)
    assert e.value.code == pkg.FMPC_E_DIM


# ------------------------------------------------------------------------------------------- 5: a recorded graph
def test_a_recorded_graph_replays_the_step_it_recorded(pkg, gpu):
    """include/fastmpc.h: the step count, the extrusion counts and the ring origins travel in the kernel arguments.  advance(1) and
    screen(...) recorded on one object and replayed once against the same calls made eagerly on its twin: the same output, the
    same windows, both one step on.  One stream, no parallel branches."""
    import torch
    W, winds, frac, n = 33, [(2.6, 1.0), (-0.3, -1.0), (-2.6, 0.3)], [0.028, 0.004, 0.008], 65
    src, a, b = (_pair(pkg, W, None, winds, frac, 17, ref=False)[0] for _ in range(3))
    mask = torch.from_numpy(_disk(n)).to(gpu)
    src.reset().advance(3)
    src.screen(n, mask=mask)                                 # (every kernel of the recording has run once before it)
    st = src.state()
    a.load_state(st); b.load_state(st)
    out_a = torch.zeros((17, n, n), dtype=torch.float64, device=gpu)
    out_b = torch.zeros_like(out_a)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.advance(1)
        a.screen(n, mask=mask, out=out_a)
    g.replay()
    b.advance(1)
    b.screen(n, mask=mask, out=out_b)
    torch.cuda.synchronize()
    sa, sb = _dev_state(a), _dev_state(b)
    assert sa["k"] == sb["k"] == st["k"] + 1 == 4 and sa["counts"] == sb["counts"] != st["counts"]
    assert torch.equal(out_a, out_b) and float(out_a.abs().max()) > 0
    assert np.array_equal(sa["windows"], sb["windows"]) and not np.array_equal(sa["windows"], st["windows"].cpu().numpy())
    for o in (src, a, b):
        o.close()


# ------------------------------------------------------------------------------------------- 6: series
def test_series_is_step_and_fit_screen_by_screen(pkg, gpu):
    """series(5, mf, skip=1, mask, scale) against a twin's five step(...) calls, each followed by mf.fit(...): the same bits, and
    the documented (batch, steps, n - skip), contiguous."""
    import torch
    op = pkg.synthetic.estimator_optics(64)
    Z = torch.from_numpy(np.ascontiguousarray(op["Z"][:10])).to(gpu)
    mf = pkg.ModalFit(Z)
    pupil = op["pupil"]
    a, b = (pkg.reference_atmosphere(4, 3, npix=32) for _ in range(2))
    a.reset(); b.reset()
    ser = a.series(5, mf, skip=1, mask=pupil, scale=0.05)
    want = torch.stack([mf.fit(b.step(64, mask=pupil, scale=0.05), skip=1).clone() for _ in range(5)], dim=1)
    torch.cuda.synchronize()
    assert tuple(ser.shape) == (4, 5, 9) and ser.is_contiguous() and ser.dtype == torch.float64
    assert torch.equal(ser, want) and a.k == b.k == 5
    assert float(ser.abs().max()) > 0 and not torch.equal(ser[:, 0], ser[:, 1])
    a.close(); b.close()
