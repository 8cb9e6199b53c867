"""fp64 iterative refinement of the fp32 factor's Schur solve (fmpc_set_refinement; fmpc_kernel_tiled.hip: ft_phase_refres,
ft_forward, ft_backward<.., true>) through the C ABI vs the structured oracle on the same seeded inputs.

With one sweep per Newton step the fp32 factor is held to the bars of the fp64 kernel (tests/test_gpu_tiled.py, _compare64):
status, ITERATION COUNTS and canonicalised line-search steps equal, z within 1e-9 relative (TOL64), nu within 1e-7.  Without
refinement the same path is only held to `iters >= oracle` and 1e-4 on z: a cold-start problem the oracle ends after one step takes
two there, which the tests below also assert, so that they exercise what they claim.

The dispatcher has no panel -> tiled (or one-wavefront -> tiled) hand-over with the fp32 factor: a handle with
FMPC_PREC_F32_MIXED goes straight to the tiled kernel for the whole batch (fmpc_solve_device_inner), and every list continuation
(FT_LIST_*) is launched with the fp64 instance.  The kernel refines list entries like any other problem, but no route reaches
that with REAL = float, so there is no test of it."""
import numpy as np
import pytest

from tests.util import canon_steps, handle_from_model, oracle_batch, rel_err

pytestmark = pytest.mark.gpu
TOL64 = 1e-9


def _solve(h, data, nw, k, z_init=None):
    return h.solve(data["x0"], data.get("x0_pre"), data.get("w"), z_init=z_init, nu0=data.get("nu0"),
                   n_newton=nw, k=k, return_info=True, check=False)


def _compare_refined(pkg, model, data, nw, k, z_init=None, sweeps=1, label=""):
    """_compare64 of tests/test_gpu_tiled.py on the fp32 factor with refinement; every figure is printed before it is asserted."""
    h = handle_from_model(pkg, model)
    h.set_precision("f32")
    h.set_refinement(sweeps)
    z, info = _solve(h, data, nw, k, z_init)
    path, _ = h.last_dispatch()
    applied = h.last_refinement()
    h.close()
    zo, nuo, ito, sto, steps = oracle_batch(model, data, nw, k, z_init=z_init)
    B = data["x0"].shape[0]
    ez = [rel_err(z[p], zo[p]) for p in range(B)]
    en = [rel_err(info["nu"][p], nuo[p]) for p in range(B)]
    print(f"refine {label} nw={nw} sweeps={sweeps}: iters {info['iters'].tolist()} oracle {list(map(int, ito))} "
          f"max rel err z {max(ez):.2e} nu {max(en):.2e}")
    assert path == pkg._lib.FMPC_PATH_TILED_F32 and applied == sweeps
    assert np.array_equal(info["status"], sto), (info["status"], sto)
    assert np.array_equal(info["iters"], ito), (info["iters"], ito)
    for p in range(B):
        assert ez[p] <= TOL64, (p, ez[p])
        assert en[p] <= 1e-7, (p, en[p])
        t = canon_steps(info["step"][p][:ito[p]])
        assert np.allclose(t, canon_steps(steps[p]), rtol=0, atol=0), (p, t, steps[p])
    return z, info, ito


def _unrefined_takes_more_steps(pkg, model, data, nw, k, ito):
    h = handle_from_model(pkg, model)
    h.set_precision("f32")
    h.set_refinement(0)
    _, info = _solve(h, data, nw, k)
    assert h.last_refinement() == 0
    h.close()
    print(f"  without refinement: iters {info['iters'].tolist()}")
    assert np.any(info["iters"] > ito), (info["iters"], ito)


@pytest.mark.parametrize("nw", [1, 3, 5])
def test_refined_fp32_ao_config_n27(pkg, gpu, nw):
    model = pkg.synthetic.make_model(27, 144, 30)
    data = pkg.synthetic.make_replay_batch(model, r=1, steps=24)
    _, _, ito = _compare_refined(pkg, model, data, nw, 1e-2, label="n=27 T=30")
    if nw == 5:
        _unrefined_takes_more_steps(pkg, model, data, nw, 1e-2, ito)


@pytest.mark.parametrize("waves", [8, 4])
@pytest.mark.parametrize("nw", [1, 3, 5])
def test_refined_fp32_config4_n65_T60(pkg, gpu, nw, waves, monkeypatch):
    """BASELINE configs[4] with 4 and with 8 wavefronts per problem (different instances of the kernel)."""
    monkeypatch.setenv("FMPC_TILED_NW", str(waves))
    model = pkg.synthetic.make_model(65, 144, 60)
    data = pkg.synthetic.make_replay_batch(model, r=4, steps=6)
    _, _, ito = _compare_refined(pkg, model, data, nw, 1e-2, label=f"n=65 T=60 waves={waves}")
    if nw == 5:
        _unrefined_takes_more_steps(pkg, model, data, nw, 1e-2, ito)


def test_refined_fp32_tight_bounds_n65(pkg, gpu):
    """Active barrier, several real Newton steps."""
    model = pkg.synthetic.make_model(65, 144, 12)
    model["u_min"] = -0.05 * np.ones(144); model["u_max"] = 0.05 * np.ones(144)
    data = pkg.synthetic.make_replay_batch(model, r=5, steps=4)
    _compare_refined(pkg, model, data, 5, 1e-2, label="tight box n=65 T=12")


@pytest.mark.parametrize("n,m,T,var,xf,sweeps", [(33, 20, 6, 2, False, 1), (40, 150, 5, 2, True, 1), (47, 60, 4, 1, False, 1),
                                                 (48, 30, 5, 2, False, 1), (63, 64, 4, 2, True, 2),
                                                 (64, 33, 4, 2, False, 1), (66, 70, 4, 1, True, 1), (79, 150, 3, 2, False, 1)])
def test_refined_fp32_random_models_over_the_block_sizes(pkg, gpu, n, m, T, var, xf, sweeps):
    """The models of test_tiled_fp32_random_models_over_the_block_sizes (run-time block structure, 3 to 5 blocks of 16) at budget 5.
    (63, 64, 4) with a terminal state (m = n + 1: the last block of Y is B W B' with a nearly square random B, the worst conditioned
    Schur system of the set) takes TWO sweeps: with one, iterations, status and steps are equal but z is 1.6e-9 and nu 1.1e-9 off
    the oracle on the device, above the 1e-9 bar."""
    from tests.test_property_random import random_problem
    model, data = random_problem(7000 + n, n, m, T, var, False, False, xf and m >= n, False, batch=4)
    _compare_refined(pkg, model, data, 5, 1e-1, sweeps=sweeps, label=f"random n={n} m={m} T={T}")


@pytest.mark.parametrize("n,m,T,var,xf", [(50, 30, 4, 2, False), (65, 70, 3, 1, True)])
def test_refined_fp32_dense_state_weights(pkg, gpu, n, m, T, var, xf):
    """Dense Q, Qf: Phi^-1 on the states inside the refinement residual is a product with (2Q)^-1, (2Qf)^-1 (XP, XfP)."""
    from tests.test_property_random import random_problem
    model, data = random_problem(8000 + n, n, m, T, var, True, False, xf and m >= n, True, batch=4)
    _compare_refined(pkg, model, data, 5, 1e-1, label=f"dense Q n={n}")


def test_refined_fp32_six_blocks_n83(pkg, gpu):
    """79 < n <= 111: fmpc_newton_tiled<float, 6, 8> (the first size of test_tiled_fp32_instances_of_six_and_seven_blocks)."""
    from tests.test_property_random import random_problem
    model, data = random_problem(400 + 83, 83, 40, 4, 2, False, False, False, True, batch=3)
    _compare_refined(pkg, model, data, 5, 1e-1, label="n=83")


def test_refined_fp32_with_disturbance_and_explicit_start(pkg, gpu):
    """w and z_init together: an off-centre start with active barrier terms (the start of the fp64 warm-start test)."""
    model = pkg.synthetic.make_model(27, 144, 10)
    model["u_min"] = -0.05 * np.ones(144); model["u_max"] = 0.05 * np.ones(144)
    data = pkg.synthetic.make_replay_batch(model, r=2, steps=8)
    rng = np.random.default_rng(7)
    data["w"] = 1e-3 * rng.standard_normal((8, 10 * 27))
    z0 = np.tile(np.concatenate([0.04 * rng.uniform(-1, 1, 144), rng.standard_normal(27)]), (8, 10))
    _compare_refined(pkg, model, data, 4, 1e-2, z_init=z0, label="w + z_init n=27 T=10")


def test_refinement_api_and_reporting(pkg, gpu):
    """Range and null-handle errors; last_refinement() tells `set` from `ran`: 0 after an fp64 solve with refinement set, the count
    after an fp32 solve."""
    lib = pkg.load()
    assert lib.fmpc_set_refinement(None, 1) == pkg._lib.FMPC_E_NULL
    assert lib.fmpc_last_refinement(None) == 0
    model = pkg.synthetic.make_model(27, 144, 6)
    data = pkg.synthetic.make_replay_batch(model, r=3, steps=5)
    h = handle_from_model(pkg, model)
    for bad in (-1, 4, 100):
        with pytest.raises(pkg.FastMPCError) as e:
            h.set_refinement(bad)
        assert e.value.code == pkg._lib.FMPC_E_DIM
    for ok in (0, 1, 2, 3):
        h.set_refinement(ok)
    assert h.last_refinement() == 0                       # nothing solved yet
    h.set_refinement(1)
    z64, _ = _solve(h, data, 3, 1e-2)                      # fp64 (the default arithmetic): the setting is ignored
    assert h.last_dispatch()[0] != pkg._lib.FMPC_PATH_TILED_F32 and h.last_refinement() == 0
    h.set_precision("f32")
    z32, _ = _solve(h, data, 3, 1e-2)
    assert h.last_dispatch()[0] == pkg._lib.FMPC_PATH_TILED_F32 and h.last_refinement() == 1
    assert max(rel_err(z32[p], z64[p]) for p in range(5)) <= TOL64
    h.set_refinement(2)
    _solve(h, data, 3, 1e-2)
    assert h.last_refinement() == 2
    h.set_precision("f64")
    _solve(h, data, 3, 1e-2)
    assert h.last_refinement() == 0
    h.close()


def test_refinement_off_is_bitwise_a_fresh_handle(pkg, gpu):
    """set_refinement(0) -- also after solves with refinement on the same handle, whose workspace slots are then the longer ones --
    gives bit for bit what a handle that never heard of refinement gives."""
    model = pkg.synthetic.make_model(65, 144, 8)
    data = pkg.synthetic.make_replay_batch(model, r=1, steps=5)
    h = handle_from_model(pkg, model)
    h.set_precision("f32")
    zf, inf_f = _solve(h, data, 3, 1e-2)
    h.close()
    h = handle_from_model(pkg, model)
    h.set_precision("f32")
    h.set_refinement(0)
    z0, inf_0 = _solve(h, data, 3, 1e-2)
    h.set_refinement(1)
    _solve(h, data, 3, 1e-2)
    h.set_refinement(0)
    z1, inf_1 = _solve(h, data, 3, 1e-2)
    h.close()
    for z, info in ((z0, inf_0), (z1, inf_1)):
        assert np.array_equal(z, zf) and np.array_equal(info["nu"], inf_f["nu"])
        assert np.array_equal(info["iters"], inf_f["iters"]) and np.array_equal(info["status"], inf_f["status"])
        assert np.array_equal(info["step"], inf_f["step"])


def test_refined_batch_beyond_grid_is_position_independent(pkg, gpu):
    """More problems than resident workgroups (grid-stride loop) with refinement: bitwise reproducible and independent of the
    problem's position in the batch (every sum of the sweeps has a fixed order)."""
    model = pkg.synthetic.make_model(27, 144, 4)
    data = pkg.synthetic.make_replay_batch(model, r=3, steps=1200)

    def run(d):
        h = handle_from_model(pkg, model)
        h.set_precision("f32")
        h.set_refinement(1)
        z, info = _solve(h, d, 2, 1e-2)
        assert h.last_dispatch()[0] == pkg._lib.FMPC_PATH_TILED_F32 and h.last_refinement() == 1
        h.close()
        return z, info["nu"]
    z1, nu1 = run(data)
    z2, nu2 = run(data)
    assert np.array_equal(z1, z2) and np.array_equal(nu1, nu2)
    perm = np.random.default_rng(0).permutation(1200)
    dperm = {k: (None if v is None else v[perm]) for k, v in data.items()}
    z3, nu3 = run(dperm)
    assert np.array_equal(z3, z1[perm]) and np.array_equal(nu3, nu1[perm])
    zo, *_ = oracle_batch(model, {k: (None if v is None else v[:5]) for k, v in data.items()}, 2, 1e-2)
    for p in range(5):
        assert rel_err(z1[p], zo[p]) <= TOL64


def test_refined_solve_recorded_into_a_graph_replays_bitwise(pkg, gpu):
    """A refined solve recorded into a HIP graph after an eager warm call (RecordedSolves makes it) replays bit for bit: the
    longer workspace slots exist before the capture, nothing is allocated under it."""
    import torch
    dev = torch.device("cuda:0")
    model = pkg.synthetic.make_model(65, 144, 10)
    d = pkg.synthetic.make_replay_batch(model, r=2, steps=12)
    h = handle_from_model(pkg, model)
    h.set_precision("f32")
    h.set_refinement(1)
    x0, x0p, nu0 = (torch.from_numpy(d[k]).to(dev) for k in ("x0", "x0_pre", "nu0"))
    z = torch.full((12, h.nz), -3.0, dtype=torch.float64, device=dev)
    nu = torch.zeros((12, d["nu0"].shape[1]), dtype=torch.float64, device=dev)
    st = torch.zeros(12, dtype=torch.int32, device=dev)
    it = torch.zeros(12, dtype=torch.int32, device=dev)

    def one():
        h.solve_device(x0, x0p, None, None, nu0, 3, 1e-2, z_out=z, nu_out=nu, status=st, iters=it)
    one()
    torch.cuda.synchronize()
    assert h.last_dispatch()[0] == pkg._lib.FMPC_PATH_TILED_F32 and h.last_refinement() == 1
    ref = (z.clone(), nu.clone(), st.clone(), it.clone())
    rec = pkg.RecordedSolves(one)
    assert rec.valid()
    for _ in range(2):
        z.fill_(-3.0); nu.fill_(0.0); st.fill_(-9); it.fill_(-9)
        rec.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, ref[0]) and torch.equal(nu, ref[1]) and torch.equal(st, ref[2]) and torch.equal(it, ref[3])
    zo, _, ito, sto, _ = oracle_batch(model, d, 3, 1e-2)
    assert np.array_equal(it.cpu().numpy(), ito) and np.array_equal(st.cpu().numpy(), sto)
    assert max(rel_err(z[p].cpu().numpy(), zo[p]) for p in range(12)) <= TOL64
    h.close()
