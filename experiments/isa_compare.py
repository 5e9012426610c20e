"""Has a change moved any kernel it was not meant to touch?  Compares the device assembly of two builds function by function (local labels
renamed in order of appearance, comments and alignment dropped) and prints, for the kernels named as excepted, the resource usage of both
builds side by side; every other function must be identical (profiles/element_layer.txt is such a record).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
          admm-elastic_amd/csrc/admm_hip.hip -o BUILD.s 2> BUILD.remarks          (once per build)
    python experiments/isa_compare.py PARENT.s THIS.s PARENT.remarks THIS.remarks k_monitor k_forces ...

The names are kernels of namespace admm_k without template arguments; all instances of a named kernel are excepted."""
import re
import shutil
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and name is None:
            name = m.group(1); body = []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body; name = None
                continue
            s = line.split(";")[0].rstrip()
            if not s.strip() or s.strip().startswith((".p2align", ".loc", ".file", ".cfi")):
                continue
            body.append(s)
    return out


def normalise(body):
    """local labels renamed in order of first appearance"""
    names = {}
    def sub(m):
        return names.setdefault(m.group(0), ".L%d" % len(names))
    return [re.sub(r"\.L[A-Za-z0-9_$.]+", sub, l) for l in body]


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    p = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.split("\n")))


def remarks(path):
    txt = open(path).read()
    res = {}
    for m in re.finditer(r"remark: [^\n]*Function Name: (\S+)(.*?)LDS Size \[bytes/block\]: (\d+)", txt, re.S):
        blk = m.group(2)
        g = lambda key: int(re.search(key + r": (\d+)", blk).group(1))
        res[m.group(1)] = dict(vgpr=g(r"VGPRs"), agpr=g(r"AGPRs"), sgpr=g(r"SGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"), occ=g(r"Occupancy \[waves/SIMD\]"),
                               lds=int(m.group(3)))
    return res


a, b = functions(sys.argv[1]), functions(sys.argv[2])
ra, rb = remarks(sys.argv[3]), remarks(sys.argv[4])
dm = demangle(sorted(set(a) | set(b)))
EXC = tuple(sys.argv[5:])
same = diff = 0
print("functions: parent %d, this %d" % (len(a), len(b)))
for n in sorted(set(a) | set(b)):
    d = dm[n]
    exc = any(("admm_k::" + e + "(") in d or ("admm_k::" + e + "<") in d for e in EXC)
    if n not in a or n not in b:
        print("ONLY IN %s: %s" % ("parent" if n in a else "this", d)); diff += 1
        continue
    eq = normalise(a[n]) == normalise(b[n])
    if exc:
        x, y = ra.get(n), rb.get(n)
        print("EXCEPTED %s: isa %s\n   parent %s\n   this   %s" % (d[:110], "same" if eq else "differs", x, y))
    elif eq:
        same += 1
    else:
        diff += 1
        print("DIFFERS (outside the scope): %s  parent %s this %s" % (d[:140], ra.get(n), rb.get(n)))
print("non-excepted functions identical: %d, different: %d" % (same, diff))
