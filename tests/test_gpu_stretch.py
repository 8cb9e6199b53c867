"""The stretch bracket (fmpc_stretch_begin / fmpc_stretch_end): consecutive cold-start steps that take the affine form are queued
and launched as chains -- one launch of fmpc_cold_affine over the steps, one flag-mode launch of the exact path with a block row
per step.  Every comparison is torch.equal against the same calls made eagerly outside a bracket, and every test asserts through
fmpc_last_stretch how many steps were fused, so none passes with the bracket doing nothing.

Shapes: (27, 144, T = 3) has 33 tiles of z; batch 90 = one full group of 64 problems + a partial one with a partial column tile,
batch 16 = one column tile.  T = 30 (321 tiles, the forms workgroups leave out their last round) once."""
import contextlib
import ctypes
import gc

import numpy as np
import pytest

from tests.util import handle_from_model

pytestmark = pytest.mark.gpu

K_BAR = 1e-2


@contextlib.contextmanager
def bracket(pkg):
    import torch
    lib = pkg._lib.load()
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.fmpc_stretch_begin(sp) == pkg._lib.FMPC_OK
    try:
        yield
    finally:
        rc = lib.fmpc_stretch_end(sp)
    assert rc == pkg._lib.FMPC_OK, rc


def make_sets(pkg, md, h, count, batch, dev, padded=False, want_z=True, scales=None, r0=30):
    import torch
    ldz = (h.nz + 15) // 16 * 16 if padded else h.nz
    sets = []
    for i in range(count):
        d = pkg.synthetic.make_replay_batch(md, r=r0 + i, steps=batch)
        sc = 1.0 if scales is None else scales[i]
        big = torch.full((batch, ldz), -3.0, dtype=torch.float64, device=dev) if want_z else None
        sets.append(dict(x0=torch.from_numpy(d["x0"] * sc).to(dev), x0p=torch.from_numpy(d["x0_pre"] * sc).to(dev), nu0=torch.from_numpy(d["nu0"]).to(dev),
                         big=big, z=None if big is None else (big[:, :h.nz] if padded else big),
                         u0=torch.zeros((batch, h.m), dtype=torch.float64, device=dev),
                         st=torch.full((batch,), -9, dtype=torch.int32, device=dev), it=torch.full((batch,), -9, dtype=torch.int32, device=dev),
                         stp=torch.zeros((batch, 1), dtype=torch.float64, device=dev)))
    return sets


OUT = ("big", "u0", "st", "it", "stp")


def solve(h, s, out=None, n_newton=1):
    o = s if out is None else out
    h.solve_device(s["x0"], s["x0p"], None, None, s["nu0"], n_newton, K_BAR, z_out=o["z"], status=o["st"], iters=o["it"], step=o["stp"] if n_newton == 1 else None,
                   u0_out=o["u0"], want_z=o["z"] is not None)


def snapshot(sets):
    import torch
    torch.cuda.synchronize()
    return [{k: s[k].clone() for k in OUT if s[k] is not None} for s in sets]


def wipe(sets):
    for s in sets:
        if s["big"] is not None:
            s["big"].fill_(-3.0)
        s["u0"].fill_(0.0); s["st"].fill_(-9); s["it"].fill_(-9); s["stp"].fill_(0.0)


def same(sets, ref):
    import torch
    torch.cuda.synchronize()
    for i, (s, r) in enumerate(zip(sets, ref)):
        for k in r:
            assert torch.equal(s[k], r[k]), (i, k)


@pytest.mark.parametrize("T,K,batch,padded,want_z", [(3, 1, 90, True, True), (3, 2, 16, False, True), (3, 5, 90, False, True), (3, 5, 90, False, False),
                                                     (3, 17, 90, True, True), (3, 16, 16, True, True), (30, 2, 90, True, True)])
def test_chain_on_disjoint_buffers_equals_eager(pkg, gpu, T, K, batch, padded, want_z):
    md = pkg.synthetic.make_model(27, 144, T)
    h = handle_from_model(pkg, md)
    sets = make_sets(pkg, md, h, K, batch, gpu, padded=padded, want_z=want_z)
    for s in sets:
        solve(h, s)
    ref = snapshot(sets)
    assert h.last_dual_form() == 2 and h.last_stretch() == (0, 0)
    wipe(sets)
    with bracket(pkg):
        for i, s in enumerate(sets):
            solve(h, s)
            # nothing is launched before the chain is full: the 17th call launches the 16 pending steps and starts a new chain
            assert h.last_stretch() == ((16, 3) if i == 16 else (0, 0)), (i, h.last_stretch())
        assert h.last_dual_form() == 2
    last = K if K <= 16 else K - 16
    assert h.last_stretch() == (last, 2 if last == 1 else (3 if want_z else 1 + last)), h.last_stretch()
    same(sets, ref)
    # and once more, mixed with a call outside the bracket
    wipe(sets)
    solve(h, sets[0])
    with bracket(pkg):
        for s in sets[1:]:
            solve(h, s)
    same(sets, ref)
    h.close()


def tight_model(pkg, T):
    md = pkg.synthetic.make_model(27, 144, T)
    md["u_min"] = -0.1 * np.ones(144); md["u_max"] = 0.1 * np.ones(144)
    return md


def test_flagged_problems_recorded_twice_then_eager(pkg, gpu):
    """Tight bounds (as the odd stretch of test_gpu_recorded.py): steps 1 and 3 hand problems to the exact path, step 2 none.  The
    chain's single flag-mode launch redoes them per block row; recorded, replayed twice back to back, then eagerly."""
    import torch
    md = tight_model(pkg, 30)
    h = handle_from_model(pkg, md)
    batch = 90
    lin = np.linspace(0.05, 5.0, batch)[:, None]
    sets = make_sets(pkg, md, h, 3, batch, gpu, scales=[lin, np.full((batch, 1), 0.01), lin], r0=20)
    handed = []
    for s in sets:
        solve(h, s); torch.cuda.synchronize(); handed.append(h.last_dispatch()[1])
    assert handed[0] > 0 and handed[2] > 0 and handed[1] == 0, handed
    ref = snapshot(sets)
    rec = pkg.RecordedSolves(lambda: [solve(h, s) for s in sets])
    assert h.last_stretch() == (3, 3)
    assert h.last_dispatch() == (pkg.FMPC_PATH_PANEL, handed[2])         # (the last step's count, as after a per-step call)
    for _ in range(2):
        wipe(sets)
        rec.replay(); rec.replay()
        same(sets, ref)
    wipe(sets)
    for s in sets:
        solve(h, s)
    same(sets, ref)
    unfused = pkg.RecordedSolves(lambda: [solve(h, s) for s in sets], fuse=False)
    assert h.last_stretch() == (3, 3)                                   # (nothing new was fused)
    wipe(sets)
    unfused.replay()
    same(sets, ref)
    h.close()


def test_four_steps_onto_one_output_tuple(pkg, gpu):
    """The later step supersedes the earlier ones: the result is the LAST call's, also for the problems an early step flagged
    and the last one did not."""
    import torch
    md = tight_model(pkg, 30)
    h = handle_from_model(pkg, md)
    batch = 90
    lin = np.linspace(0.05, 5.0, batch)[:, None]
    sets = make_sets(pkg, md, h, 4, batch, gpu, scales=[lin, 0.5 * lin, np.full((batch, 1), 0.01), lin[::-1].copy()], r0=20)
    out = sets[0]
    handed, redone = [], []
    for s in sets:
        solve(h, s, out); torch.cuda.synchronize()
        handed.append(h.last_dispatch()[1]); redone.append(out["stp"][:, 0] != 1.0)
    assert handed[0] > 0 and handed[3] > 0, handed
    assert bool((redone[0] & ~redone[3]).any()), "no problem that step 1 hands over and step 4 does not: the case tests nothing"
    ref = snapshot([out])
    wipe([out])
    with bracket(pkg):
        for s in sets:
            solve(h, s, out)
    assert h.last_stretch() == (4, 2)                                   # (one live step: one flag-mode launch)
    same([out], ref)
    assert h.last_dispatch()[1] == handed[3]
    h.close()


def test_overlapping_buffers_launch_the_pending_chain_first(pkg, gpu):
    import torch
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    batch = 90
    sets = make_sets(pkg, md, h, 3, batch, gpu)
    # (a) step 2 writes the first moves of step 1 again but another z: neither disjoint nor identical
    mixed = dict(sets[1]); mixed["u0"] = sets[0]["u0"]
    # (b) step 3 reads its x0 from the z step 2 has written
    chained = dict(sets[2]); chained["x0"] = sets[1]["big"].view(-1)[:batch * 27].view(batch, 27)

    def calls(check):
        solve(h, sets[0]); check(0)
        solve(h, sets[1], mixed); check(1)
        solve(h, chained); check(2)

    calls(lambda i: None)
    ref = snapshot(sets)
    wipe(sets)
    seen = []
    with bracket(pkg):
        calls(lambda i: seen.append(h.last_stretch()))
    assert seen == [(0, 0), (1, 2), (1, 2)] and h.last_stretch() == (1, 2), seen    # three chains of one step
    same(sets, ref)
    h.close()


def test_other_call_between_two_steps_keeps_the_order(pkg, gpu):
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    batch = 16
    sets = make_sets(pkg, md, h, 2, batch, gpu)

    def calls():
        solve(h, sets[0])
        solve(h, sets[0], n_newton=3)           # a budget of 3 is no affine step; it overwrites what the first call wrote
        solve(h, sets[1])

    calls()
    ref = snapshot(sets)
    assert h.last_stretch() == (0, 0)
    wipe(sets)
    with bracket(pkg):
        calls()
    assert h.last_stretch() == (1, 2)
    same(sets, ref)
    h.close()


def test_foreign_work_under_capture_fails_cleanly(pkg, gpu):
    """A torch kernel between two bracketed solves of a capturing stream should have run after a step that is not enqueued yet:
    the second solve refuses (FMPC_E_UNSUPPORTED), the pending step is dropped, the capture ends cleanly, nothing was allocated,
    and the handle solves eagerly afterwards as a fresh one does."""
    import torch
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    batch = 90
    sets = make_sets(pkg, md, h, 2, batch, gpu)
    for s in sets:
        solve(h, s)
    ref = snapshot(sets)
    wipe(sets)
    torch.cuda.synchronize()
    lib = pkg._lib.load()
    gen = int(lib.fmpc_alloc_generation())
    other = torch.zeros(64, dtype=torch.float64, device=gpu)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    gc.collect()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                sp = ctypes.c_void_p(side.cuda_stream)
                assert lib.fmpc_stretch_begin(sp) == pkg._lib.FMPC_OK
                solve(h, sets[0])
                other.fill_(1.0)
                with pytest.raises(pkg.FastMPCError) as ei:
                    solve(h, sets[1])
                assert lib.fmpc_stretch_end(sp) == pkg._lib.FMPC_OK      # (the chain was dropped: nothing is pending)
    finally:
        gc.enable()
    torch.cuda.synchronize()
    assert ei.value.code == pkg._lib.FMPC_E_UNSUPPORTED
    assert int(lib.fmpc_alloc_generation()) == gen
    assert h.last_stretch() == (0, 0)
    # RecordedSolves names the way out
    with pytest.raises(pkg.FastMPCError, match="fuse=False") as e2:
        pkg.RecordedSolves(lambda: (solve(h, sets[0]), other.fill_(1.0), solve(h, sets[1])))
    assert e2.value.code == pkg._lib.FMPC_E_UNSUPPORTED
    wipe(sets)
    for s in sets:
        solve(h, s)
    same(sets, ref)
    h.close()


def test_residual_screen_behind_a_bracketed_solve(pkg, gpu):
    """fmpc_phase_residual_device reads the first moves a queued step has yet to write (the solve -> residual screen sequence of
    AOLoop.step): the pending chain is launched first, the screen equals the eager one."""
    import torch
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    batch, npx = 16, 200
    sets = make_sets(pkg, md, h, 2, batch, gpu)
    rng = np.random.default_rng(5)
    phase = torch.from_numpy(rng.standard_normal((batch, npx))).to(gpu)
    Z = torch.from_numpy(rng.standard_normal((27, npx))).to(gpu)
    out = torch.zeros((batch, npx), dtype=torch.float64, device=gpu)
    lib = pkg._lib.load()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())

    def calls():
        solve(h, sets[0])
        solve(h, sets[1])
        sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.fmpc_phase_residual_device(h._h, batch, npx, vp(phase), vp(sets[1]["u0"]), vp(Z), vp(out), sp) == pkg._lib.FMPC_OK

    calls()
    ref = snapshot(sets)
    ref_out = out.clone()
    assert float(ref_out.abs().max()) > 0.0 and not torch.equal(ref_out, phase)
    wipe(sets); out.zero_()
    with bracket(pkg):
        calls()
        assert h.last_stretch() == (2, 3)                               # (launched by the residual call, not by the end)
    same(sets, ref)
    assert torch.equal(out, ref_out)
    h.close()


def test_two_chains_with_flagged_problems_in_one_graph(pkg, gpu):
    """Two chains in ONE recorded graph, both with problems for the exact path, in other steps and other problems: the second
    chain's flag-mode launch has to see ITS parameter blocks (device memory the launch before it rewrites), not the first's."""
    import torch
    md = tight_model(pkg, 30)
    h = handle_from_model(pkg, md)
    lin = lambda b: np.linspace(0.05, 5.0, b)[:, None]
    few = lambda b: np.full((b, 1), 0.01)
    first = make_sets(pkg, md, h, 3, 90, gpu, scales=[lin(90), few(90), lin(90)[::-1].copy()], r0=20)
    second = make_sets(pkg, md, h, 3, 80, gpu, scales=[few(80), lin(80), lin(80)], r0=40)      # (another batch: another chain)
    handed = []
    for s in first + second:
        solve(h, s); torch.cuda.synchronize(); handed.append(h.last_dispatch()[1])
    assert handed[0] > 0 and handed[2] > 0 and handed[4] > 0 and handed[5] > 0 and handed[1] == 0 and handed[3] == 0, handed
    ref = snapshot(first + second)
    seen = []

    def stretch():
        for s in first:
            solve(h, s)
        for s in second:
            solve(h, s); seen.append(h.last_stretch())
    rec = pkg.RecordedSolves(stretch)
    assert seen[:3] == [(3, 3)] * 3 and h.last_stretch() == (3, 3), seen       # (the first chain was launched by the 4th call)
    for _ in range(2):
        wipe(first + second)
        rec.replay(); rec.replay()
        same(first + second, ref)
    h.close()
