"""Do the instances of the tiled Newton kernel that existed before a change still disassemble as they did?

    python scripts/compare_tiled_disassembly.py OLD/fmpc_kernel_tiled.o NEW/fmpc_kernel_tiled.o

Both arguments are objects of csrc/fmpc_kernel_tiled.hip (lib/obj/fmpc_kernel_tiled.o of a build of the older and of the newer
tree).  The gfx950 code object is taken out of each, disassembled, and every function of the older one is compared, instruction
by instruction, with the function of the same name in the newer one; trailing template arguments that the newer tree added with
the value `false` (the model-bank flag BK, the empty FtSel<false> argument) are dropped from its names first, and instances with
such an argument `true` are new and skipped -- unless the older tree has a function of exactly the same name (both trees have
the bank instances), which is then the one compared.  PC-relative literals (the s_add_u32 / s_addc_u32 pair behind s_getpc_b64 that
forms a callee's address) move with the code layout and are masked.  Also compares the kernels' register and scratch totals
(what -Rpass-analysis=kernel-resource-usage prints) from the code objects' metadata.  Needs /opt/rocm/llvm/bin and c++filt."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")


def code_object(obj, tmp, tag):
    fb, co = os.path.join(tmp, tag + ".fb"), os.path.join(tmp, tag + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fb], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fb, "--output=" + co, "--unbundle"], check=True)
    return co


def functions(co):
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    fn = collections.OrderedDict(); cur = None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = m.group(1); fn[cur] = []
            continue
        if cur is None or not line.strip():
            continue
        t = line.split("//")[0].strip()
        t = re.sub(r"<[^>]*>", "<sym>", t)
        t = re.sub(r"^(s_add_u32|s_addc_u32) (s\d+), (s\d+), 0x[0-9a-f]{5,}$", r"\1 \2, \3, REL", t)
        fn[cur].append(t)
    for body in fn.values():                                # the padding behind a function's last instruction is not part of it
        while body and (body[-1] in ("s_code_end", "...") or body[-1].startswith("s_nop")):
            body.pop()
    return fn


def resources(co):
    text = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for blk in text.split("- .agpr_count:")[1:]:
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        out[g("name")] = dict(vgpr=int(g("vgpr_count")), agpr=int(re.match(r"\s*(\d+)", blk).group(1)), sgpr=int(g("sgpr_count")),
                              scratch=int(g("private_segment_fixed_size")), spills=int(g("vgpr_spill_count")))
    return out


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def key(d):
    return re.sub(r"\s+", "", d)


def new_key(d):
    """Name of a function of the newer tree as the older tree spelt it, or None for an instance that is new."""
    d = key(d)
    if "FtSel<true>" in d or (d.startswith("voidfmpc_newton_tiled<") and d.endswith(",true>(FtParams)")):
        return None
    d = d.replace(",FtSel<false>", "").replace("FtSel<false>", "")
    if re.match(r"^(FtResid|FtStep|void|bool)(ft_phase_|fmpc_newton_tiled)", d):
        d = re.sub(r",false>\(", ">(", d, count=1)
    return d


def main():
    old_obj, new_obj = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        oco, nco = code_object(old_obj, tmp, "old"), code_object(new_obj, tmp, "new")
        O, N = functions(oco), functions(nco)
        RO, RN = resources(oco), resources(nco)
    do, dn = demangle(list(O)), demangle(list(N))
    newer = {}
    for k, v in dn.items():
        nk = new_key(v)
        if nk is not None:
            newer[nk] = k
    for k, v in dn.items():                                 # both trees spell the name alike (both have the bank instances): that wins
        newer[key(v)] = k
    same = differ = missing = moved = 0
    for k, v in do.items():
        nk = newer.get(key(v))
        if nk is None:
            missing += 1; print("MISSING ", v)
            continue
        if O[k] == N[nk]:
            same += 1
        else:
            differ += 1
            nd = sum(1 for x, y in zip(O[k], N[nk]) if x != y) + abs(len(O[k]) - len(N[nk]))
            print(f"DIFFERS  {v}: {len(O[k])} -> {len(N[nk])} instructions, {nd} differ")
        if k in RO and nk in RN and RO[k] != RN[nk]:
            moved += 1; print(f"RESOURCES {v}: {RO[k]} -> {RN[nk]}")
    print(f"functions of the older object: {len(O)}; same {same}, differ {differ}, missing {missing}; kernels whose resource totals moved: {moved}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
