"""Device assembly of every HIP source in two trees, compared: python tools/isa_diff.py BASE_TREE [files...]

For a "same code, moved" change to the kernels: BASE_TREE is an export of the parent commit (git archive HEAD~1 | tar -x -C DIR).
Each file is compiled with the build's flags plus --offload-device-only -S, from its own csrc/ directory so that embedded
file names agree.  Prints `identical` or the number of differing lines per file, and for a differing file the register /
scratch / LDS figures of each kernel on both sides (from the assembly's metadata).  A differing file is `reordered only`
when every kernel keeps those four figures and every function keeps its multiset of instruction mnemonics (a moved
instruction, commuted operands, renumbered labels), else it has `different instructions`; exit status 1 if any file has."""
import collections
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIP_SOURCES, HIPCC_FLAGS  # noqa: E402

KEYS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def assemble(tree, src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # -cuid: the compilation unit id (a __hip_cuid_<hash> symbol) is otherwise a hash of the file's absolute path
    p = subprocess.run([hipcc] + HIPCC_FLAGS + ["--offload-device-only", "-S", "-cuid=" + src, src, "-o", out],
                       cwd=os.path.join(tree, "openseg3d_amd", "csrc"), capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src} in {tree}\n{p.stderr}")
    with open(out) as f:
        return f.read().splitlines()


def kernel_figures(lines):
    """{kernel: {key: value}} from the amdhsa.kernels metadata at the end of the assembly"""
    text = "\n".join(lines)
    text = text[text.find("amdhsa.kernels:"):]
    figures = {}
    for entry in re.split(r"\n  - ", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry)
        if name:
            figures[name.group(1)] = {k: v for k, v in re.findall(r"(\.\w+):\s+(\d+)\s*(?:\n|$)", entry) if k in KEYS}
    return figures


def mnemonics(lines):
    """{function: Counter of its instruction mnemonics} for the kernels and the device functions that were not inlined"""
    out, cur = {}, None
    for line in lines:
        start = re.match(r"(\S+):\s+; @", line)
        if start:
            cur = out.setdefault(start.group(1), collections.Counter())
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line.startswith("\t"):
            word = line.split(None, 1)[0] if line.strip() else "."
            if word[0] not in ".;":  # directives and comments
                cur[word] += 1
    return out


def main():
    base, files = os.path.abspath(sys.argv[1]), sys.argv[2:] or HIP_SOURCES
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(min(16, os.cpu_count())) as pool:
        jobs = [(src, pool.submit(assemble, base, src, os.path.join(tmp, "base_" + src + ".s")),
                 pool.submit(assemble, ROOT, src, os.path.join(tmp, "work_" + src + ".s"))) for src in files]
        changed = 0
        for src, a, b in jobs:
            a, b = a.result(), b.result()
            n = sum(1 for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[0] in "+-" and d[:3] not in ("+++", "---"))
            fa, fb = kernel_figures(a), kernel_figures(b)
            moved = fa == fb and mnemonics(a) == mnemonics(b)
            verdict = "identical" if n == 0 else f"{n} differing lines, " + ("reordered only" if moved else "different instructions")
            print(f"{src:28s} {verdict}  ({len(b)} lines)", flush=True)
            if n:
                changed += 0 if moved else 1
                for k in sorted(set(fa) | set(fb)):
                    print(f"    {k}")
                    for key in KEYS:
                        print(f"        {key:30s} {fa.get(k, {}).get(key, '-'):>8s} -> {fb.get(k, {}).get(key, '-'):>8s}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
