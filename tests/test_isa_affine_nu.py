"""Static check of the hand-counted memory waits of `fmpc_cold_nu` (csrc/fmpc_kernel_affine_nu.hip): the walk of
tests/test_isa_affine_hazard.py -- gfx950's one in-order counter for loads and stores, every loop once more around its back-edge --
over the kernels of the new file.  The operand requests are chained through the three phases of an item (direct tiles, nu+, u tiles)
and every one is awaited before the item ends; no instruction may touch a register with a load in flight, and the kernels use no
scratch.  Nothing else is looked for in the assembly."""
import os
import re
import shutil
import subprocess

import pytest

from test_isa_affine_hazard import HIPCC, ROOT, _parse, check_kernel

SRC = os.path.join(ROOT, "mpc-sensorlessao_amd", "csrc", "fmpc_kernel_affine_nu.hip")


@pytest.fixture(scope="module")
def nu_asm(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / "affine_nu.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, SRC],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return open(out).read()


def test_nu_kernels_have_no_scratch_and_no_register_touched_under_a_load_in_flight(nu_asm):
    kernels = _parse(nu_asm)
    assert len(kernels) == 2, list(kernels)                      # non-temporal stores or not
    assert not any("fmpc_cold_affine" in k for k in kernels)     # (the fixed checks of the other file's kernels do not apply here)
    for blk in re.findall(r"\.amdhsa_kernel\s+\S+.*?\.end_amdhsa_kernel", nu_asm, flags=re.S):
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", blk), "the kernel uses scratch"
    assert not re.search(r"\bscratch_(load|store)", "\n".join("%s %s" % (op, a) for k in kernels for _, op, a in kernels[k] if op))
    for k, ins in kernels.items():
        errs = check_kernel(k, ins)
        assert not errs, "\n".join(errs[:10])
