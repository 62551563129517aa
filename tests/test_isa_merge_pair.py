"""What the compiler makes of k_bpe_merge_lds_pair (CPU only: `hipcc -S` for gfx950, no GPU) -- tests/test_isa.py's checks of the merge
kernels, for the kernel that runs both of their bodies in one launch, and the resources its launch shape depends on: two 640-lane
workgroups per CU are five wavefronts per SIMD, which leaves 96 vector registers, and the 32-symbol body must fit them without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIR = ("tkamd::k_bpe_merge_lds_pair<true>", "tkamd::k_bpe_merge_lds_pair<false>")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp_path_factory.mktemp("isa_pair") / "kernels.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DTKAMD_BUILD", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "tokenizers_amd", "csrc", "kernels.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    s = open(out).read()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_ZN5tkamd\w+):", s, re.M)]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in starts), capture_output=True, text=True).stdout.split("\n")
    by_name = {}
    for (pos, mangled), d in zip(starts, names):
        body = s[pos:s.find(".Lfunc_end", pos)].split("\n")
        ins = [l.strip() for l in body if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        k = s.find(".amdhsa_kernel " + mangled)
        desc = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", s[k:s.find(".end_amdhsa_kernel", k)])) if k >= 0 else {}
        by_name[d.split("(")[0].replace("void ", "")] = (ins, desc)
    return by_name


def runs(ins, prefix):
    """lengths of the runs of instructions starting with `prefix` with no s_waitcnt vmcnt and no branch between them"""
    out, cur = [], 0
    for l in ins:
        if l.startswith(prefix):
            cur += 1
        elif l.startswith(("s_waitcnt vmcnt", "s_cbranch", "s_branch", "s_barrier")):
            if cur:
                out.append(cur)
            cur = 0
    return out + ([cur] if cur else [])


def roles(ins):
    """The kernel's two unit bodies, each from its counting sort's histogram atomic (the one LDS add whose result is used) to the next:
    {symbols: (instructions, index of the first instruction behind the merge loop's minimum tree)}.  The tree is what tells them
    apart: v_min3 over 31 keys is 15 instructions, over 15 keys 7."""
    cuts = [i for i, l in enumerate(ins) if l.startswith("ds_add_rtn_u32")] + [len(ins)]
    out = {}
    for a, b in zip(cuts, cuts[1:]):
        body = ins[a:b]
        mins = [i for i, l in enumerate(body) if l.startswith("v_min3_u32")]
        if mins:
            assert mins[-1] - mins[0] < 60, "one minimum tree per unit body"
            out[{15: 32, 7: 16}[len(mins)]] = (body, mins[-1] + 1)
    return out


@pytest.mark.parametrize("name", PAIR)
def test_pair_kernel_probes(asm, name):
    ins, _ = asm[name]
    assert not any(l.startswith("flat_load") for l in ins), name + ": a flat load (a run-time LDS-or-memory pointer) waits for everything in flight"
    r = roles(ins)
    assert sorted(r) == [16, 32], name + ": both unit bodies are in the kernel"
    for sym, (body, behind_tree) in r.items():
        who = "%s, %d-symbol role" % (name, sym)
        # The first probes go in groups of eight (the last group: seven), S / 8 groups.  tests/test_isa.py asks ONE group of k_bpe_merge_lds
        # to leave with no wait inside it -- with the displacements in memory the compiler cuts a body's first group by partial waits --;
        # here every group behind the first must, in each role by itself
        assert sum(1 for n in runs(body, "global_load_dwordx3") if n >= 7) >= sym // 8 - 1, who + ": the first probes of a word leave eight at a time"
        # the merge loop: behind the minimum tree the next two probes are the merge's two new pairs -- no wait between them
        loads = [i for i in range(behind_tree, len(body)) if body[i].startswith("global_load_dwordx3")][:2]
        assert len(loads) == 2 and loads[1] - behind_tree < 400, who + ": the merge's two probes follow the minimum tree"
        assert not any(l.startswith("s_waitcnt vmcnt") for l in body[loads[0]:loads[1]]), who + ": the two probes of a merge are in flight together"


@pytest.mark.parametrize("name", PAIR)
def test_pair_kernel_fits_two_workgroups_per_cu(asm, name):
    ins, desc = asm[name]
    assert not any(l.startswith("scratch_") for l in ins), name + ": spills"
    assert int(desc["private_segment_fixed_size"]) == 0, desc
    assert int(desc["next_free_vgpr"]) <= 96, desc            # five wavefronts per SIMD of 512 registers, allocated in eights
    assert not any("accvgpr" in l for l in ins), name + ": spills to the accumulation registers"
    # static LDS (two prefix arrays) + the dynamic part of the displacement-cached instantiation, twice, within a CU's 160 KB
    dyn = (16 * 640 + 256 + 64) * 4 + 16384 * 2
    assert 2 * (int(desc["group_segment_fixed_size"]) + dyn) <= 160 * 1024, desc
