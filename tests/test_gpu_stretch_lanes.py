"""Lanes of a chain (fmpc_host_plan_lanes, fmpc_cold_affine): the steps of a bracketed stretch that write different output tuples
run side by side in the one launch, each (lane, group of 64 problems) on its own share of the workgroups; the steps of one
tuple stay in one lane, in order.  Every comparison is torch.equal against the same calls made eagerly outside a bracket, and
every test asserts through fmpc_last_stretch how many steps were fused.

Shapes: (27, 144, T = 3) has 33 tiles of z (+ 6 of nu+); batch 90 = one full group of 64 problems + a partial one with a partial
column tile: two groups, so K steps on distinct buffers are K lanes with the 9 workgroups per group of one tile per wavefront.
T = 30 (321 tiles) once."""
import numpy as np
import pytest

from tests.test_gpu_stretch import K_BAR, bracket, tight_model
from tests.test_host_lane_plan import plan, sup_of
from tests.util import handle_from_model

pytestmark = pytest.mark.gpu

OUT = ("big", "nu", "u0", "st", "it", "stp")


def make_sets(pkg, md, h, count, batch, dev, padded=False, want_z=True, want_nu=False, scales=None, r0=30, one_batch=False):
    import torch
    ldz = (h.nz + 15) // 16 * 16 if padded else h.nz
    sets, d = [], None
    for i in range(count):
        if d is None or not one_batch:
            d = pkg.synthetic.make_replay_batch(md, r=r0 + i, steps=batch)
        sc = (1.0 + 0.03 * i if one_batch else 1.0) if scales is None else scales[i]
        big = torch.full((batch, ldz), -3.0, dtype=torch.float64, device=dev) if want_z else None
        sets.append(dict(x0=torch.from_numpy(d["x0"] * sc).to(dev), x0p=torch.from_numpy(d["x0_pre"] * sc).to(dev), nu0=torch.from_numpy(d["nu0"]).to(dev),
                         big=big, z=None if big is None else (big[:, :h.nz] if padded else big),
                         nu=torch.full((batch, h.nu_len), -5.0, dtype=torch.float64, device=dev) if want_nu else None,
                         u0=torch.zeros((batch, h.m), dtype=torch.float64, device=dev),
                         st=torch.full((batch,), -9, dtype=torch.int32, device=dev), it=torch.full((batch,), -9, dtype=torch.int32, device=dev),
                         stp=torch.zeros((batch, 1), dtype=torch.float64, device=dev)))
    return sets


def solve(h, s, out=None):
    o = s if out is None else out
    h.solve_device(s["x0"], s["x0p"], None, None, s["nu0"], 1, K_BAR, z_out=o["z"], nu_out=o["nu"], status=o["st"], iters=o["it"], step=o["stp"],
                   u0_out=o["u0"], want_z=o["z"] is not None)


def snapshot(sets):
    import torch
    torch.cuda.synchronize()
    return [{k: s[k].clone() for k in OUT if s[k] is not None} for s in sets]


def wipe(sets):
    for s in sets:
        for k, v in (("big", -3.0), ("nu", -5.0), ("u0", 0.0), ("st", -9), ("it", -9), ("stp", 0.0)):
            if s[k] is not None:
                s[k].fill_(v)


def same(sets, ref):
    import torch
    torch.cuda.synchronize()
    for i, (s, r) in enumerate(zip(sets, ref)):
        for k in r:
            assert torch.equal(s[k], r[k]), (i, k)


def slots_of(gpu):
    import torch
    return 2 * torch.cuda.get_device_properties(gpu).multi_processor_count


@pytest.mark.parametrize("K", [5, 16])
@pytest.mark.parametrize("padded,want_z,want_nu", [(True, True, False), (False, True, False), (True, True, True), (False, True, True), (False, False, False)])
def test_distinct_buffers_run_in_lanes(pkg, gpu, K, padded, want_z, want_nu):
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    tiles = ((h.nz + 15) // 16 + ((h.nu_len + 15) // 16 if want_nu else 0)) if want_z else (h.m + 15) // 16
    assert plan(sup_of(list(range(K))), 2, slots_of(gpu), tiles) == (K, (tiles + 3) // 4, list(range(K)))    # K lanes, wpg at its clamp
    sets = make_sets(pkg, md, h, K, 90, gpu, padded=padded, want_z=want_z, want_nu=want_nu)
    for s in sets:
        solve(h, s)
    ref = snapshot(sets)
    assert h.last_dual_form() == 2 and h.last_stretch() == (0, 0)
    wipe(sets)
    with bracket(pkg):
        for s in sets:
            solve(h, s)
    assert h.last_stretch() == (K, 3 if want_z else 1 + K), h.last_stretch()
    same(sets, ref)
    h.close()


def interleaved(pkg, gpu, T=3):
    """Six steps on two output tuples in the order A, B, A, B, A, A, every step with inputs of its own; tight bounds, so that steps
    hand problems to the exact path -- an early step of A others than the last one."""
    md = tight_model(pkg, T)
    h = handle_from_model(pkg, md)
    batch = 90
    lin = np.linspace(0.05, 5.0, batch)[:, None]
    few = np.full((batch, 1), 0.01)
    sets = make_sets(pkg, md, h, 6, batch, gpu, padded=True, scales=[lin, 0.7 * lin, 0.5 * lin, few, few, lin[::-1].copy()], r0=20)
    outs = [sets[0], sets[1], sets[0], sets[1], sets[0], sets[0]]
    return h, sets, outs


def test_interleaved_classes_keep_their_order(pkg, gpu, monkeypatch):
    import torch
    h, sets, outs = interleaved(pkg, gpu)
    handed, redone = [], []
    for s, o in zip(sets, outs):
        solve(h, s, o); torch.cuda.synchronize()
        handed.append(h.last_dispatch()[1]); redone.append(o["stp"][:, 0] != 1.0)
    print("handed per step:", handed)
    assert handed[0] > 0 and handed[1] > 0 and handed[5] > 0, handed
    assert bool((redone[0] & ~redone[5]).any()) and bool((redone[1] & ~redone[3]).any()), "no problem an early step hands over and the tuple's last does not"
    ref = snapshot(sets[:2])
    assert plan(sup_of([0, 1, 0, 1, 0, 0]), 2, slots_of(gpu), 33)[0::2] == (2, [0, 1, 0, 1, 0, 0])
    results = []
    for cap in (None, "1"):
        if cap is None:
            monkeypatch.delenv("FMPC_STRETCH_LANES", raising=False)
        else:
            monkeypatch.setenv("FMPC_STRETCH_LANES", cap)
        wipe(sets[:2])
        with bracket(pkg):
            for s, o in zip(sets, outs):
                solve(h, s, o)
        assert h.last_stretch() == (6, 3), h.last_stretch()            # (two live steps: one flag-mode launch with two block rows)
        same(sets[:2], ref)
        results.append(snapshot(sets[:2]))
    same(sets[:2], results[0])
    for a, b in zip(results[0], results[1]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert h.last_dispatch()[1] == handed[5]
    h.close()


def test_one_workgroup_per_step_and_group_then_merged_lanes(pkg, gpu):
    """16 steps on distinct buffers at 64 slots / 16 problems: exactly `slots` (step, group) pairs -- 16 lanes of ONE workgroup per group
    (8 rounds of 4 tiles, the 33rd tile by column tile).  One group more and the lanes have to merge."""
    md = pkg.synthetic.make_model(27, 144, 3)
    h = handle_from_model(pkg, md)
    slots = slots_of(gpu)
    ngroups = slots // 16
    assert plan(sup_of(list(range(16))), ngroups, slots, 33)[:2] == (16, 1)
    lanes, wpg, lane_of = plan(sup_of(list(range(16))), ngroups + 1, slots, 33)
    assert 1 < lanes < 16 and max(lane_of.count(l) for l in range(lanes)) >= 2                 # (at 512 slots: 4 lanes of 4 steps, wpg = 3)
    for batch in (64 * ngroups, 64 * ngroups + 64):
        sets = make_sets(pkg, md, h, 16, batch, gpu, padded=True, one_batch=True)
        for s in sets:
            solve(h, s)
        ref = snapshot(sets)
        wipe(sets)
        with bracket(pkg):
            for s in sets:
                solve(h, s)
        assert h.last_stretch() == (16, 3), h.last_stretch()
        same(sets, ref)
        del sets, ref
    h.close()


def test_long_horizon_in_four_lanes(pkg, gpu):
    """T = 30: 321 tiles on 4 lanes x 2 groups -- 64 workgroups per group, a count a single step never has (one round of 256 tiles,
    65 tiles by column tile)."""
    md = pkg.synthetic.make_model(27, 144, 30)
    h = handle_from_model(pkg, md)
    slots = slots_of(gpu)
    assert plan(sup_of([0, 1, 2, 3]), 2, slots, 321)[:2] == (4, min(slots // 8, 81))
    sets = make_sets(pkg, md, h, 4, 90, gpu, padded=True)
    for s in sets:
        solve(h, s)
    ref = snapshot(sets)
    wipe(sets)
    with bracket(pkg):
        for s in sets:
            solve(h, s)
    assert h.last_stretch() == (4, 3), h.last_stretch()
    same(sets, ref)
    h.close()


def test_recorded_interleaved_classes(pkg, gpu):
    import torch
    h, sets, outs = interleaved(pkg, gpu)
    for s, o in zip(sets, outs):
        solve(h, s, o)
    ref = snapshot(sets[:2])
    rec = pkg.RecordedSolves(lambda: [solve(h, s, o) for s, o in zip(sets, outs)])
    assert h.last_stretch() == (6, 3), h.last_stretch()
    for _ in range(2):
        wipe(sets[:2])
        rec.replay(); rec.replay()
        same(sets[:2], ref)
    wipe(sets[:2])
    for s, o in zip(sets, outs):
        solve(h, s, o)
    same(sets[:2], ref)
    h.close()
