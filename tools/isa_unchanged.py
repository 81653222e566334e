"""Every kernel of a base commit compiles to the same gfx950 instructions in the working tree.

Builds the device code of every .hip file of lidarshooter_amd/csrc twice -- as of BASE (git archive) and as in the working
tree -- with the Makefile's flags and -S --cuda-device-only, and compares, kernel by kernel, the instruction text of every
kernel that exists in the base (labels renumbered, directives and comments dropped).  New kernels are listed, not compared.
usage: python tools/isa_unchanged.py [BASE]     (BASE: a commit, default HEAD)   exit 0 = unchanged, 1 = a kernel differs
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-Wno-unused-result"]


def kernels(asm_path):
    """mangled name -> instruction lines of its body"""
    src = open(asm_path).read().split("\n")
    out, name, body = {}, None, []
    for line in src:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", t):
                body.append("label")
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", "L", t))
    return out


def build(tree, out_dir):
    csrc = os.path.join(tree, "lidarshooter_amd", "csrc")
    res = {}
    # the translation units: the Makefile's kernel objects (a .hip without one -- ls_standing.hip -- is compiled as part of another)
    units = set(re.search(r"^KERN_OBJ\s*:=(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1).split())
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith(".hip") or fn[:-4] + ".o" not in units:
            continue
        asm = os.path.join(out_dir, fn + ".s")
        subprocess.check_call([HIPCC, "--offload-arch=gfx950", *FLAGS, "-S", "--cuda-device-only", "-o", asm, os.path.join(csrc, fn)])
        for k, v in kernels(asm).items():
            res[k] = (fn, v)
    return res


def main():
    base = sys.argv[1] if len(sys.argv) > 1 else "HEAD"
    tmp = tempfile.mkdtemp(prefix="isa_unchanged_")
    try:
        btree = os.path.join(tmp, "base")
        os.makedirs(btree)
        arch = subprocess.check_output(["git", "-C", ROOT, "archive", base, "lidarshooter_amd/csrc", "include"])
        subprocess.run(["tar", "-x", "-C", btree], input=arch, check=True)
        os.makedirs(os.path.join(tmp, "b"))
        os.makedirs(os.path.join(tmp, "h"))
        before = build(btree, os.path.join(tmp, "b"))
        after = build(ROOT, os.path.join(tmp, "h"))
        bad = 0
        for k in sorted(before):
            fn, body = before[k]
            if k not in after:
                print(f"MISSING  {k} ({fn})")
                bad += 1
            elif after[k][1] != body:
                print(f"CHANGED  {k} ({fn}): {len(body)} -> {len(after[k][1])} instructions")
                bad += 1
        for k in sorted(set(after) - set(before)):
            print(f"new      {k} ({after[k][0]}, {len(after[k][1])} instructions)")
        print(f"{len(before)} kernels of {base}: {len(before) - bad} identical, {bad} differ")
        return 1 if bad else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
