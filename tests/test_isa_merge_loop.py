"""What one iteration of the merge loop of k_bpe_merge_lds_pair costs in vector instructions (CPU only: `hipcc -S` for gfx950, no GPU).

A launch of the pair kernel lasts as long as its longest word's chain of dependent merges, and a wavefront shares its SIMD's vector
issue with the wavefronts beside it: the vector instructions of one iteration of the merge loop (`do .. while (__any(active))`) are
what every merge of the chain pays.  With the symbols in registers most of them were the select chains of the dynamic indices and the
copies of the symbol registers around the loop's `if`s -- 369 vector instructions an iteration in the 32-symbol role and 217 in the
16-symbol role, with a linear chain of compare + conditional move per register.  The binary select trees must stay below both
figures, in both instantiations of the kernel (the displacements in LDS and in memory).

The loop is found in the ISA as the innermost branch back over the unit body's minimum tree that has the merge's two probes inside
(tests/test_isa_merge_pair.py tells the two bodies apart by that tree), together with the blocks the compiler laid out in front of
the loop's header: from the first of them to the back edge, every instruction of the loop counted once.
`python tests/test_isa_merge_loop.py` prints the counts."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
PAIR = ("tkamd::k_bpe_merge_lds_pair<true>", "tkamd::k_bpe_merge_lds_pair<false>")
LINEAR_CHAIN_VALU = {32: 369, 16: 217}          # one iteration with the linear select chains


def compile_kernels(out):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DTKAMD_BUILD", "--cuda-device-only", "-S",
                        os.path.join(ROOT, "tokenizers_amd", "csrc", "kernels.hip"), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(out).read()


def kernel_lines(s, name):
    """instructions and labels of the kernel whose demangled name starts with `name`"""
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(_ZN5tkamd\w+):", s, re.M)]
    names = subprocess.run(["c++filt"], input="\n".join(n for _, n in starts), capture_output=True, text=True).stdout.split("\n")
    for (pos, _), d in zip(starts, names):
        if d.split("(")[0].replace("void ", "") == name:
            body = s[pos:s.find(".Lfunc_end", pos)].split("\n")
            return [l.strip() if l.startswith("\t") else l.split(":")[0] + ":" for l in body
                    if re.match(r"\.LBB\w+:", l) or (l.startswith("\t") and not l.strip().startswith((".", ";")))]
    raise AssertionError(name + " is not in the ISA")


def merge_loops(lines):
    """{symbols of the role: the lines of its merge loop, branch target to back edge}"""
    cuts = [i for i, l in enumerate(lines) if l.startswith("ds_add_rtn_u32")] + [len(lines)]
    out = {}
    for a, b in zip(cuts, cuts[1:]):
        mins = [i for i in range(a, b) if lines[i].startswith("v_min3_u32")]
        if not mins:
            continue
        role = {15: 32, 7: 16}[len(mins)]
        label_at = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
        best = None
        for i in range(mins[-1], b):
            m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", lines[i])
            if m and label_at.get(m.group(1), len(lines)) < mins[0] and label_at[m.group(1)] >= a:
                span = (label_at[m.group(1)], i)
                # (the loop of the merges, not a wait loop inside it: the one with the merge's two probes)
                if sum(l.startswith("global_load_dwordx3") for l in lines[span[0]:span[1]]) >= 2 and (best is None or span[1] - span[0] < best[1] - best[0]):
                    best = span
        assert best, "no branch back over the minimum tree of the %d-symbol role" % role
        # (the compiler lays blocks of the loop -- the ends of its `if`s -- out in front of the loop's header: every block of this unit
        # body that a branch of the loop goes back to belongs to it)
        lo, hi = best
        while True:
            targets = [label_at.get(m.group(1), hi) for m in (re.match(r"s_c?branch\w*\s+(\.LBB\w+)", l) for l in lines[lo:hi + 1]) if m]
            new_lo = min([p for p in targets if a <= p < lo], default=lo)
            if new_lo == lo:
                break
            lo = new_lo
        out[role] = lines[lo:hi + 1]
    return out


def counts(loop):
    ins = [l for l in loop if not l.endswith(":")]
    return {"valu": sum(l.startswith("v_") for l in ins), "salu": sum(l.startswith("s_") and not l.startswith("s_waitcnt") for l in ins),
            "lds": sum(l.startswith("ds_") for l in ins), "probes": sum(l.startswith("global_load_dwordx3") for l in ins),
            "waitcnt": sum(l.startswith("s_waitcnt") for l in ins),
            "cmp_cndmask": sum(l.startswith(("v_cmp", "v_cndmask")) for l in ins)}


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    return compile_kernels(str(tmp_path_factory.mktemp("isa_loop") / "kernels.s"))


@pytest.mark.parametrize("name", PAIR)
def test_an_iteration_is_cheaper_than_with_linear_select_chains(asm, name):
    loops = merge_loops(kernel_lines(asm, name))
    assert sorted(loops) == [16, 32], name + ": both unit bodies have a merge loop"
    for role, loop in loops.items():
        c = counts(loop)
        print(name, role, c)
        assert c["probes"] == 2, (name, role, c)                       # (the loop that was found is the merge loop: its two probes)
        assert c["valu"] < LINEAR_CHAIN_VALU[role], (name, role, c)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        text = compile_kernels(os.path.join(d, "kernels.s")) if len(sys.argv) < 2 else open(sys.argv[1]).read()
    for name in PAIR:
        for role, loop in sorted(merge_loops(kernel_lines(text, name)).items()):
            print(name, "%d-symbol role:" % role, counts(loop))
