#!/usr/bin/env python3
"""Is the device code of csrc/kernels.hip the same in two source trees, kernel for kernel?  For a change to the launchers or to host code that must leave
every kernel as it is.  Each tree's kernels.hip is compiled to device assembly twice, with the command of its own Makefile rule (build/kernels.o and the
-DMI355RT_WIDE=1 build/kernels_wide.o) plus --cuda-device-only -S, and the two sides are compared PER FUNCTION SYMBOL, not as files: the order in which template
instantiations are emitted follows their first use in the launchers and moves with them.  Per symbol the text is: the function's section of the assembly and
its entry of the amdhsa.kernels metadata, without comment lines and trailing comments, with the numbers of the local labels (.LBB<n>_, .Lfunc_begin<n>,
.Lfunc_end<n>, .Ltmp<n>: emission order) replaced by their rank of first appearance and the __hip_cuid_<hash> symbol (source hash) by its bare name.  Texts are
hashed and compared; nothing is looked for in them.  Also compared: the sorted rows of each tree's tools/kernel_resources.py, and, where both trees hold them,
the objects of the other kernel files (build/lbvh.o, bake.o, probes.o, probes_vis.o) byte for byte.
usage: tools/kernel_identity.py <treeA> <treeB>      exit status 0: identical"""
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "raytracer-rs_amd"
OTHER_OBJECTS = ["lbvh.o", "bake.o", "probes.o", "probes_vis.o"]
LABEL = re.compile(r"\.(LBB|Lfunc_begin|Lfunc_end|Ltmp)(\d+)")


def device_asm(tree, wide, out):
    pkg = os.path.join(tree, PKG)
    target = "build/kernels_wide.o" if wide else "build/kernels.o"
    dry = subprocess.run(["make", "-n", "-W", "csrc/kernels.hip", target], cwd=pkg, capture_output=True, text=True, check=True).stdout
    cmd = shlex.split([l for l in dry.splitlines() if "csrc/kernels.hip" in l and " -c " in l][0])
    cmd = cmd[:cmd.index("-o")] + cmd[cmd.index("-o") + 2:]
    cmd[cmd.index("-c")] = "-S"
    subprocess.run(cmd + ["--cuda-device-only", "-o", out], cwd=pkg, check=True)
    return open(out).read()


def normalise(lines):
    rank, out = {}, []
    for line in lines:
        line = line.split(";", 1)[0].rstrip()
        if not line:
            continue
        line = LABEL.sub(lambda m: ".%s#%d" % (m.group(1), rank.setdefault(m.group(0), len(rank))), line)
        out.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", line))
    return "\n".join(out)


def split(asm):
    """{symbol: normalised text}, set of kernel symbols.  '' holds what belongs to no function (the module's head, tail and metadata frame)."""
    head = []
    parts, kernels, cur, meta, item, items = {}, set(), head, False, None, []
    for line in asm.splitlines():
        m = re.search(r"; -- Begin function (\S+)", line)
        if cur is head and re.match(r"\s*\.(text|section)\b", line):
            cur = []                                            # the module's head ends at the first section directive
        if m:                                                   # what came since the function before (the section directive of an instantiation) is this one's
            parts[m.group(1)] = cur
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            kernels.add(m.group(1))
        if line.strip() in (".amdgpu_metadata", ".end_amdgpu_metadata"):
            meta, item = line.strip() == ".amdgpu_metadata", None
        elif meta and line.startswith("  - "):                  # an entry of amdhsa.kernels: its .name says whose it is
            item = []
            items.append(item)
        elif item is not None and not line.startswith("    "):
            item = None
        (cur if item is None else item).append(line)
        if re.match(r"\s*\.section\s+\.AMDGPU\.csdata", line):     # the last directive of a function
            cur = []
    parts[""] = head + cur                                      # behind the last function: the module's tail
    for item in items:
        names = [m.group(1) for m in (re.match(r"\s*\.name:\s*(\S+)", l) for l in item) if m]
        parts[names[0] if names else ""] += item
    return {k: normalise(v) for k, v in parts.items()}, kernels


def resources(tree, wide):
    r = subprocess.run([sys.executable, os.path.join(tree, "tools", "kernel_resources.py")] + (["-DMI355RT_WIDE=1"] if wide else []), capture_output=True, text=True)
    return sorted(r.stdout.splitlines()) if r.returncode == 0 else None


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    trees = [os.path.abspath(t) for t in sys.argv[1:]]
    differing = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(4) as pool:
        asm = {(t, w): pool.submit(device_asm, trees[t], w, os.path.join(tmp, "%d%d.s" % (t, w))) for t in (0, 1) for w in (0, 1)}
        res = {(t, w): resources(trees[t], w) for t in (0, 1) for w in (0, 1)}       # one at a time: the tool writes a fixed temporary
        for w in (0, 1):
            (a, ka), (b, kb) = split(asm[(0, w)].result()), split(asm[(1, w)].result())
            diff = sorted(s for s in set(a) & set(b) if a[s] != b[s])
            digest = [hashlib.sha256("".join(sorted(hashlib.sha256(v.encode()).hexdigest() + k for k, v in x.items())).encode()).hexdigest()[:16] for x in (a, b)]
            variants = [sum(1 for k in ks if re.search(r"(trace_kernel|shade_kernel|resolve_kernel)I", k)) for ks in (ka, kb)]
            print("%s build (%s):" % ("wide" if w else "normal", "-DMI355RT_WIDE=1" if w else "the Makefile's flags"))
            print("  kernel symbols: A %d, B %d; of them trace_kernel / shade_kernel / resolve_kernel variants: A %d, B %d" % (len(ka), len(kb), variants[0], variants[1]))
            print("  function symbols: A %d, B %d; only in A: %d, only in B: %d; normalised text differs: %d" % (len(a) - 1, len(b) - 1, len(set(a) - set(b)), len(set(b) - set(a)), len(diff)))
            print("  digest over all per-symbol hashes: A %s, B %s" % tuple(digest))
            for s in sorted((set(a) ^ set(b)) | set(diff)):
                print("    %s %s" % ("differs:" if s in diff else "only in A:" if s in a else "only in B:", s or "(module head and tail)"))
            ra, rb = res[(0, w)], res[(1, w)]
            same_rows = ra is not None and ra == rb
            print("  tools/kernel_resources.py: A %s rows, B %s rows, %s" % (ra and len(ra) - 1, rb and len(rb) - 1, "identical" if same_rows else "NOT identical"))
            differing += len(diff) + len(set(a) ^ set(b)) + (ka != kb) + (not same_rows)
    for o in OTHER_OBJECTS:
        pa, pb = (os.path.join(t, PKG, "build", o) for t in trees)
        if os.path.exists(pa) and os.path.exists(pb):
            same = open(pa, "rb").read() == open(pb, "rb").read()
            print("build/%s: %s" % (o, "byte-identical" if same else "DIFFERS"))
            differing += not same
    print("identical" if not differing else "NOT identical: %d findings" % differing)
    sys.exit(1 if differing else 0)


if __name__ == "__main__":
    main()
