"""GPU tests of the affine cold-start step with the u rows through nu+ (csrc/fmpc_kernel_affine_nu.hip): every call that writes z.
FMPC_AFFINE_DIRECT=1 (read at every launch) selects fmpc_cold_affine, every tile as one product over d: the reference in the same
process.  Stage 0 and every tile with x rows are computed by the same instruction sequence in both kernels, so the first moves are
bit for bit the same; the u rows of the stages 1 .. T-1 go through nu+ and agree within the bar the project sets between two
evaluations of this step, rel_err <= 1e-11 per problem (tests/test_gpu_affine.py).  Measured on an MI355X, worst over the cases below:
7.1e-16 (T = 30, batch 2000; 3.5e-16 .. 4.5e-16 at the smaller shapes).

Shapes, the smallest that reach every branch: T = 3 (stages at offsets 0, 11, 6 of a tile: an item with 8 u tiles and a tile across
the block boundary on both sides); T = 30 once at batch 90 (the other residues, stage 16 on a tile boundary with 9 u tiles); batch 16
(one column tile), 90 (a full group and a partial one: both store paths of the u tiles) and 2000 once (two parts per item); terminal
row on and off, VAR(1), nu_out on and off, padded and contiguous rows.  Between themselves the forms of the new kernel are bit for
bit equal: a chain of 1, 2, 5, 16 steps and per-step calls, 4 lanes and one, padded and contiguous rows, with and without nu_out,
the first-moves-only call and z[:, :m].  T = 2 at batch 8256 once: at most 3 workgroups per group, where a workgroup evaluates the
decision forms of two column tiles in turn."""
import numpy as np
import pytest

from tests.test_gpu_stretch import K_BAR, bracket
from tests.test_gpu_stretch_lanes import make_sets, same, snapshot, solve, wipe
from tests.util import canon_steps, handle_from_model, oracle_batch, rel_err

pytestmark = pytest.mark.gpu


def _run(h, t, batch, dev, padded=False, want_nu=False, want_z=True):
    import torch
    ldz = (h.nz + 15) // 16 * 16 if padded else h.nz
    big = torch.full((batch, ldz), -7.0, dtype=torch.float64, device=dev) if want_z else None
    z = None if big is None else big[:, :h.nz]
    u0 = torch.full((batch, h.m), float("nan"), dtype=torch.float64, device=dev)
    st = torch.full((batch,), -99, dtype=torch.int32, device=dev); it = torch.full((batch,), -99, dtype=torch.int32, device=dev)
    stp = torch.full((batch, 1), float("nan"), dtype=torch.float64, device=dev)
    nu = torch.full((batch, h.nu_len), float("nan"), dtype=torch.float64, device=dev) if want_nu else None
    h.solve_device(t["x0"], t["x0_pre"], None, None, t["nu0"], 1, K_BAR, z_out=z, nu_out=nu, status=st, iters=it, step=stp, u0_out=u0, want_z=want_z)
    torch.cuda.synchronize()
    assert h.last_dual_form() == 2
    if padded and want_z:
        assert bool((big[:, h.nz:] == -7.0).all()), "something was written between the rows"
    return dict(z=None if z is None else z.cpu().numpy(), u0=u0.cpu().numpy(), st=st.cpu().numpy(), it=it.cpu().numpy(), stp=stp.cpu().numpy(),
                nu=None if nu is None else nu.cpu().numpy())


@pytest.mark.parametrize("T,batch,xf,var_order", [
    (3, 16, False, 2),
    (3, 90, True, 2),
    (3, 90, False, 1),               # VAR(1): x0_pre = NULL
    (30, 90, False, 2),
    (30, 2000, False, 2),            # 64 wavefronts per group: two parts per item
])
def test_u_rows_through_nu_match_the_direct_product(pkg, gpu, monkeypatch, T, batch, xf, var_order):
    import torch
    md = pkg.synthetic.make_model(27, 144, T, var_order=var_order)
    rng = np.random.default_rng(5)
    if xf:
        md["xf"] = 0.01 * rng.standard_normal(27)
    data = pkg.synthetic.make_replay_batch(md, r=5, steps=batch)
    data["w"] = None
    data["nu0"] = rng.standard_normal((batch, (T + (1 if xf else 0)) * 27))
    if var_order == 1:
        data["x0_pre"] = None
    h = handle_from_model(pkg, md)
    t = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(gpu)) for k, v in data.items()}
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    a = _run(h, t, batch, gpu)
    monkeypatch.setenv("FMPC_AFFINE_DIRECT", "1")
    d = _run(h, t, batch, gpu)
    dn = _run(h, t, batch, gpu, want_nu=True)
    monkeypatch.delenv("FMPC_AFFINE_DIRECT")
    assert np.array_equal(a["st"], d["st"]) and np.array_equal(a["it"], d["it"]) and np.array_equal(a["stp"], d["stp"])
    assert np.all(np.isfinite(a["z"])) and np.array_equal(a["z"][:, :144], d["z"][:, :144])
    worst = max(rel_err(a["z"][p], d["z"][p]) for p in range(batch))
    print("T = %d, batch = %d: worst rel_err of z against the direct product %.3e" % (T, batch, worst))
    assert worst <= 1e-11
    assert not np.array_equal(a["z"], d["z"]) or T == 1            # (the switch does select another kernel)
    nchk = min(batch, 6)
    sub = {k: (v[:nchk] if v is not None else None) for k, v in data.items()}
    zo, _, ito, sto, steps = oracle_batch(md, sub, 1, K_BAR)
    assert np.array_equal(a["it"][:nchk], ito) and np.array_equal(a["st"][:nchk], sto)
    assert np.array_equal(canon_steps(a["stp"][:nchk, 0]), canon_steps([s[0] for s in steps]))
    assert max(rel_err(a["z"][p], zo[p]) for p in range(nchk)) <= 1e-9
    # between themselves the forms are bit for bit equal: padded rows, with nu_out (whose rows are direct tiles: those of the
    # direct kernel), the first moves, and the first-moves-only call (which stays on fmpc_cold_affine)
    assert np.array_equal(a["u0"], a["z"][:, :144])
    for padded, want_nu in ((True, False), (False, True), (True, True)):
        b = _run(h, t, batch, gpu, padded=padded, want_nu=want_nu)
        assert np.array_equal(b["z"], a["z"]) and np.array_equal(b["u0"], a["u0"]) and np.array_equal(b["st"], a["st"]), (padded, want_nu)
        if want_nu:
            assert np.array_equal(b["nu"], dn["nu"])
    uo = _run(h, t, batch, gpu, want_z=False)
    assert np.array_equal(uo["u0"], a["u0"]) and np.array_equal(uo["st"], a["st"]) and np.array_equal(uo["it"], a["it"])
    h.close()


def test_a_workgroup_with_two_column_tiles_of_decision_forms(pkg, gpu, monkeypatch):
    """At most 3 workgroups per group: one workgroup evaluates the decision forms of two column tiles in turn (fa_forms walks
    fct = wpg - 1 - slot, += wpg) and reuses sF behind the barrier -- in a call that WRITES z through fmpc_cold_affine<true, .>.
    (27, 144, 2) at batch 8256: 129 groups on the 512 workgroup slots of 256 compute units.  Both kernels decide alike; z within
    the bar of test_u_rows_through_nu_match_the_direct_product; the first-moves-only call is bit for bit the direct call's z[:, :m].
    Measured on an MI355X: no problem handed to the exact path, worst rel_err of z 9.3e-16."""
    import torch
    from tests.test_host_lane_plan import plan
    T, batch = 2, 8256
    md = pkg.synthetic.make_model(27, 144, T)
    h = handle_from_model(pkg, md)
    ngroups = (batch + 63) // 64
    slots = 2 * torch.cuda.get_device_properties(gpu).multi_processor_count
    for tiles in ((h.nz + 15) // 16, (h.m + 15) // 16):               # the call that writes z, the first-moves-only call
        lanes, wpg, _ = plan([0], ngroups, slots, tiles, cap=1)
        assert lanes == 1 and wpg <= 3, (lanes, wpg, slots)
    data = pkg.synthetic.make_replay_batch(md, r=7, steps=batch)
    scale = np.linspace(0.5, 50.0, batch)[:, None]                  # (measured: every problem is accepted at t = 1, z is the affine kernels')
    data["x0"] = data["x0"] * scale; data["x0_pre"] = data["x0_pre"] * scale
    data["w"] = None
    t = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(gpu)) for k, v in data.items()}
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    a = _run(h, t, batch, gpu)
    handed = h.last_dispatch()[1]
    monkeypatch.setenv("FMPC_AFFINE_DIRECT", "1")
    d = _run(h, t, batch, gpu)
    assert h.last_dispatch()[1] == handed
    uo = _run(h, t, batch, gpu, want_z=False)
    assert h.last_dispatch()[1] == handed
    monkeypatch.delenv("FMPC_AFFINE_DIRECT")
    print("batch %d: %d problems handed to the exact path" % (batch, handed))
    assert handed < batch, "every problem was redone by the exact path: z of the affine kernels is not compared"
    for key in ("st", "it", "stp"):
        assert np.array_equal(a[key], d[key]) and np.array_equal(uo[key], d[key]), key
    assert np.all(np.isfinite(a["z"])) and np.all(np.isfinite(d["z"]))
    worst = float(np.max(np.linalg.norm(a["z"] - d["z"], axis=1) / np.linalg.norm(d["z"], axis=1)))      # rel_err per problem
    print("worst rel_err of z against the direct product %.3e" % worst)
    assert worst <= 1e-11
    assert np.array_equal(d["u0"], d["z"][:, :144]) and np.array_equal(uo["u0"], d["z"][:, :144])
    h.close()


@pytest.mark.parametrize("K", [1, 2, 5, 16])
def test_chain_equals_per_step_calls_in_lanes_and_in_one(pkg, gpu, monkeypatch, K):
    """K steps on distinct padded buffers inside a bracket: K lanes; FMPC_STRETCH_LANES=1: one after another.  Both bit for bit the
    per-step calls (which, at batch 90 and T = 3, run 9 workgroups per group where a lane of the chain has fewer)."""
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    sets = make_sets(pkg, md, h, K, 90, gpu, padded=True, want_nu=(K == 5))
    for s in sets:
        solve(h, s)
    ref = snapshot(sets)
    for cap in (None, "1"):
        if cap is None:
            monkeypatch.delenv("FMPC_STRETCH_LANES", raising=False)
        else:
            monkeypatch.setenv("FMPC_STRETCH_LANES", cap)
        wipe(sets)
        with bracket(pkg):
            for s in sets:
                solve(h, s)
        if K > 1:
            assert h.last_stretch()[0] == K, h.last_stretch()
        same(sets, ref)
    h.close()


def test_four_lanes_at_the_long_horizon(pkg, gpu, monkeypatch):
    """T = 30 at batch 90 in 4 lanes against one lane and against per-step calls: other workgroups per group, other parts per item."""
    monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
    md = pkg.synthetic.make_model(27, 144, 30)
    h = handle_from_model(pkg, md)
    sets = make_sets(pkg, md, h, 4, 90, gpu, padded=True)
    for s in sets:
        solve(h, s)
    ref = snapshot(sets)
    for cap in (None, "1"):
        if cap is None:
            monkeypatch.delenv("FMPC_STRETCH_LANES", raising=False)
        else:
            monkeypatch.setenv("FMPC_STRETCH_LANES", cap)
        wipe(sets)
        with bracket(pkg):
            for s in sets:
                solve(h, s)
        assert h.last_stretch() == (4, 3), h.last_stretch()
        same(sets, ref)
    h.close()


def test_flagged_problems_end_with_the_exact_paths_z(pkg, gpu, monkeypatch):
    """Tight bounds, as tests/test_gpu_affine.py builds the hand-over: at +-0.05 (T = 10) every problem is flagged and redone by the
    exact path, which overwrites z -- bit for bit what it leaves behind the direct kernel; at +-0.1 (T = 3, the model of
    tests/test_gpu_stretch.py) flagged and accepted problems sit side by side."""
    import torch
    for ub, T, want_all in ((0.05, 10, True), (0.1, 3, False)):
        md = pkg.synthetic.make_model(27, 144, T)
        md["u_min"] = -ub * np.ones(144); md["u_max"] = ub * np.ones(144)
        batch = 70
        data = pkg.synthetic.make_replay_batch(md, r=3, steps=batch)
        data["x0"] = data["x0"] * np.linspace(0.05, 5.0, batch)[:, None]
        data["x0_pre"] = data["x0_pre"] * np.linspace(0.05, 5.0, batch)[:, None]
        data["w"] = None
        h = handle_from_model(pkg, md)
        t = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(gpu)) for k, v in data.items()}
        monkeypatch.delenv("FMPC_AFFINE_DIRECT", raising=False)
        a = _run(h, t, batch, gpu)
        handed = h.last_dispatch()[1]
        monkeypatch.setenv("FMPC_AFFINE_DIRECT", "1")
        d = _run(h, t, batch, gpu)
        assert h.last_dispatch()[1] == handed
        monkeypatch.delenv("FMPC_AFFINE_DIRECT")
        print("bounds +-%.2f: %d of %d problems handed to the exact path" % (ub, handed, batch))
        assert handed == batch if want_all else 0 < handed < batch
        assert np.array_equal(a["st"], d["st"]) and np.array_equal(a["it"], d["it"]) and np.array_equal(a["stp"], d["stp"])
        assert np.array_equal(a["u0"], a["z"][:, :144]) and np.array_equal(a["u0"], d["u0"])
        redone = a["stp"][:, 0] != 1.0                              # (certainly handed over: the affine kernel only ever accepts t = 1)
        if want_all:
            assert redone.any(), "no backtracking in the tight-box case"
            assert np.array_equal(a["z"], d["z"])
        assert np.array_equal(a["z"][redone], d["z"][redone])
        assert max(rel_err(a["z"][p], d["z"][p]) for p in range(batch)) <= 1e-11
        pick = [0, batch // 2, batch - 1]
        sub = {k: (v[pick] if v is not None else None) for k, v in data.items()}
        zo, _, ito, sto, _ = oracle_batch(md, sub, 1, K_BAR)
        assert np.array_equal(a["it"][pick], ito) and np.array_equal(a["st"][pick], sto)
        assert max(rel_err(a["z"][p], zo[q]) for q, p in enumerate(pick)) <= 1e-9
        h.close()
