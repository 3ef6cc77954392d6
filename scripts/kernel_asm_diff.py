#!/usr/bin/env python3
"""Compares the device assembly of two csrc trees kernel by kernel (CPU only:
hipcc cross-compiles).  The proof a source-moving refactor gives: every
kernel's code and kernel descriptor unchanged, wherever its source now lives.

  usage: scripts/kernel_asm_diff.py OLD_CSRC NEW_CSRC [-j JOBS] [-v]

Each tree must sit where its Makefile's relative include paths resolve (for
the old one: a worktree of the older commit).  Every compile command of
`make -n -B all` is rerun with --offload-device-only -S; the output is cut
per kernel symbol (its label to the function's end, and its .amdhsa_kernel
block), comments and .p2align / .loc / .file lines are dropped and the
.LBB<function index>_ label prefix becomes .LBB_ (the index is the kernel's
position in its file).  Kernels are matched by mangled name across the whole
tree.  Prints the kernels per file, the kernels only one tree has, and every
kernel whose code or descriptor differs, with its registers, scratch, LDS and
instruction count on both sides.  Exit status 1 when a kernel both trees have
differs, 0 otherwise.  Only kernel symbols are compared: a __device__ function
that is not inlined into its callers lies outside every compared body."""
import argparse
import concurrent.futures
import difflib
import os
import re
import shlex
import subprocess
import sys
import tempfile

RES = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
       ("scratch", ".amdhsa_private_segment_fixed_size"),
       ("lds", ".amdhsa_group_segment_fixed_size"))


def compile_commands(csrc):
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, "all"], check=True,
                         capture_output=True, text=True).stdout
    cmds = []
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and "-o" in argv:
            cmds.append(argv)
    if not cmds:
        sys.exit("no compile commands from make -n in %s" % csrc)
    return cmds


def device_asm(csrc, argv, tmp):
    src = argv[argv.index("-c") + 1]
    dst = os.path.join(tmp, src + ".s")
    argv = list(argv)
    argv[argv.index("-o") + 1] = dst
    subprocess.run(argv + ["--offload-device-only", "-S"], check=True, cwd=csrc,
                   capture_output=True, text=True)
    with open(dst) as f:
        return src, f.read()


def normalise(lines):
    out = []
    for l in lines:
        l = l.split(";", 1)[0].strip()
        if not l or l.split()[0] in (".p2align", ".loc", ".file"):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", l))
    return out


def kernels_of(text):
    """{mangled name: (code lines, descriptor lines)} of one assembly file."""
    lines = text.splitlines()
    desc = {}
    i = 0
    while i < len(lines):
        w = lines[i].split()
        if len(w) == 2 and w[0] == ".amdhsa_kernel":
            j = i
            while lines[j].strip() != ".end_amdhsa_kernel":
                j += 1
            desc[w[1]] = normalise(lines[i:j + 1])
            i = j
        i += 1
    res = {}
    for i, l in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", l)
        if m and m.group(1) in desc:
            j = i + 1
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            res[m.group(1)] = (normalise(lines[i + 1:j]), desc[m.group(1)])
    missing = set(desc) - set(res)
    if missing:
        sys.exit("no code found for %s" % sorted(missing))
    return res


def tree(csrc, jobs):
    """{name: (file, code, descriptor)} and {file: kernel count}."""
    cmds = compile_commands(csrc)
    kern, per_file = {}, {}
    with tempfile.TemporaryDirectory() as tmp, \
            concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        for src, text in pool.map(lambda a: device_asm(csrc, a, tmp), cmds):
            ks = kernels_of(text)
            per_file[src] = len(ks)
            for name, (code, desc) in ks.items():
                if name in kern:
                    sys.exit("%s is in %s and %s" % (name, kern[name][0], src))
                kern[name] = (src, code, desc)
    return kern, per_file


def resources(code, desc):
    r = {}
    for key, directive in RES:
        r[key] = next(int(l.split()[1], 0) for l in desc if l.split()[0] == directive)
    r["instr"] = sum(1 for l in code if not l.endswith(":") and not l.startswith("."))
    return r


def demangle(names):
    try:
        out = subprocess.run(["llvm-cxxfilt"] + names, check=True, capture_output=True, text=True,
                             env=dict(os.environ, PATH=os.environ.get("PATH", "") +
                                      ":/opt/rocm/llvm/bin")).stdout.splitlines()
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def literals_only(a, b):
    """The two listings differ only in numeric literals (e.g. the offset of an
    s_getpc-relative constant table: layout, not code)."""
    num = re.compile(r"\b(0x[0-9a-fA-F]+|\d+)\b")
    return len(a) == len(b) and all(num.sub("#", x) == num.sub("#", y) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("-v", "--verbose", action="store_true", help="print the diff of differing kernels")
    a = ap.parse_args()
    old, old_files = tree(a.old_csrc, a.jobs)
    new, new_files = tree(a.new_csrc, a.jobs)
    for tag, files in (("old", old_files), ("new", new_files)):
        print("%s: %d kernels; per file: %s" % (
            tag, sum(files.values()),
            ", ".join("%s %d" % (f, c) for f, c in sorted(files.items()) if c)))
    names = demangle(sorted(set(old) | set(new)))
    for tag, only, src in (("old", set(old) - set(new), old), ("new", set(new) - set(old), new)):
        for n in sorted(only):
            print("only in %s (%s): %s  %s" % (tag, src[n][0], names[n], resources(*src[n][1:])))
    same = differ = 0
    for n in sorted(set(old) & set(new)):
        (fo, co, do), (fn, cn, dn) = old[n], new[n]
        if co == cn and do == dn:
            same += 1
            continue
        differ += 1
        what = [w for w, x, y in (("code", co, cn), ("descriptor", do, dn)) if x != y]
        if co != cn and do == dn and literals_only(co, cn):
            what = ["numeric literals only"]
        print("DIFFERS (%s) %s -> %s: %s\n  old %s\n  new %s" % (
            ", ".join(what), fo, fn, names[n], resources(co, do), resources(cn, dn)))
        if a.verbose:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(co + do, cn + dn, "old", "new",
                                                                         n=1, lineterm=""))
    print("%d kernels in both trees: %d identical in code and descriptor, %d differ" % (
        same + differ, same, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
