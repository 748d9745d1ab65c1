"""Instruction-level comparison of the GPU kernels of two source trees: did a refactor leave the kernels alone?

usage: python scripts/isa_compare.py TREE_A TREE_B --a attention.hip --b attention.hip attention_fwd.hip ... [--arch gfx950]

Each named file of olmoasr_amd/csrc is compiled device-only to assembly with the flags its tree's Makefile gives that file's object
(`make -n`), and the result is split per kernel symbol.  Per kernel the report compares
  * the sequence of instruction mnemonics (labels, directives and comments dropped),
  * the .amdhsa_* resource directives (VGPR / AGPR / SGPR counts, LDS bytes, scratch bytes, ...).
Instructions at the same position whose mnemonics agree but whose operands differ are counted in two classes: the same operands in
another order (v_add_f32 v1, v2, v3 against v_add_f32 v1, v3, v2), and anything else (another register, another immediate).
Exit status 0: same kernel symbols, same mnemonic sequences, same resource directives."""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("olmoasr_amd", "csrc")


def compile_command(tree, src, arch):
    """The compiler line of `make build/<src>.o`, as a list, with its -c / -o parts taken off."""
    obj = "build/" + os.path.splitext(src)[0] + ".o"
    out = subprocess.run(["make", "-n", "-B", "ARCH=" + arch, obj], cwd=os.path.join(tree, CSRC), check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        words = shlex.split(line)
        if "-c" in words and src in words:
            i = words.index("-o")
            del words[i:i + 2]
            words.remove("-c")
            words.remove(src)
            return words
    raise SystemExit(f"{tree}: no compile line for {obj} in the Makefile's dry run")


def assemble(tree, src, arch, tmp):
    out = os.path.join(tmp, src + ".s")
    cmd = compile_command(tree, src, arch) + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")


def kernels_of(asm):
    """{symbol: (instructions [(mnemonic, [operands])], {directive: value})} of one assembly file."""
    lines = asm.splitlines()
    res = {}
    name = None
    for ln in lines:  # resource directives
        s = ln.strip()
        if s.startswith(".amdhsa_kernel "):
            name = s.split()[1]
            res[name] = {}
        elif s == ".end_amdhsa_kernel":
            name = None
        elif name and s.startswith(".amdhsa_"):
            k, _, v = s.partition(" ")
            res[name][k] = v.strip()
    body = {}
    cur = None
    for ln in lines:  # code between `symbol:` and its .Lfunc_end label
        m = LABEL.match(ln)
        if m:
            if m.group(1) in res:
                cur = body.setdefault(m.group(1), [])
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            continue
        if cur is None:
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            continue
        mnem, _, ops = s.partition(" ")
        cur.append((mnem, [o.strip() for o in ops.split(",")] if ops.strip() else []))
    return {k: (body.get(k, []), res[k]) for k in res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--a", nargs="+", required=True, help=".hip files of TREE_A's csrc")
    ap.add_argument("--b", nargs="+", required=True, help=".hip files of TREE_B's csrc")
    ap.add_argument("--arch", default="gfx950")
    args = ap.parse_args()

    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for tag, tree, files in (("a", args.tree_a, args.a), ("b", args.tree_b, args.b)):
            ks = {}
            os.mkdir(os.path.join(tmp, tag))
            for f in files:
                flags = " ".join(w for w in compile_command(tree, f, args.arch)[1:] if not w.startswith("-W"))
                print(f"{tag}: {f}: {flags}")
                for k, v in kernels_of(assemble(tree, f, args.arch, os.path.join(tmp, tag))).items():
                    if k in ks:
                        raise SystemExit(f"{tree}: kernel {k} defined twice")
                    ks[k] = v + (f,)
            sides.append(ks)
    ka, kb = sides
    bad = 0
    for k in sorted(set(ka) - set(kb)):
        print(f"ONLY IN A  {k}")
        bad += 1
    for k in sorted(set(kb) - set(ka)):
        print(f"ONLY IN B  {k}")
        bad += 1
    print(f"\n{len(set(ka) & set(kb))} kernel symbols in both trees")
    for k in sorted(set(ka) & set(kb)):
        (ia, ra, fa), (ib, rb, fb) = ka[k], kb[k]
        same_seq = [m for m, _ in ia] == [m for m, _ in ib]
        swapped = other = 0
        first = None
        if same_seq:
            for (m, oa), (_, ob) in zip(ia, ib):
                if oa != ob:
                    if sorted(oa) == sorted(ob):
                        swapped += 1
                    else:
                        other += 1
        else:
            n = min(len(ia), len(ib))
            first = next((i for i in range(n) if ia[i][0] != ib[i][0]), n)
        res_diff = {d: (ra.get(d), rb.get(d)) for d in sorted(set(ra) | set(rb)) if ra.get(d) != rb.get(d)}
        ok = same_seq and not res_diff
        bad += not ok
        print(f"\n{'SAME' if ok else 'DIFF'}  {k}\n      {fa} -> {fb}")
        print(f"      instructions {len(ia)} / {len(ib)}: mnemonic sequence {'equal' if same_seq else f'DIFFERS from instruction {first}'}")
        if same_seq:
            print(f"      operands: {swapped} in another order, {other} otherwise different")
        res_keys = (".amdhsa_next_free_vgpr", ".amdhsa_accum_offset", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")
        print("      resources: " + ("equal" if not res_diff else "DIFFER") + f" ({len(ra)} directives); " +
              ", ".join(f"{d[8:]} {ra.get(d)}" for d in res_keys if d in ra))
        for d, (x, y) in res_diff.items():
            print(f"      {d}: {x} -> {y}")
    print(f"\n{'OK' if not bad else 'FAILED'}: {bad} difference(s) in kernel symbols, mnemonic sequences or resource directives")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
