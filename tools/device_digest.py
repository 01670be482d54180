"""Digest of the DEVICE code of every .hip source of libmipme, to show that a host-side change left the kernels alone:
    python tools/device_digest.py [csrc directory ...]        (default: torch-pme_amd/csrc of this checkout)
Each source is compiled for the device only, with the Makefile's flags, and three views of the code object are hashed: the
disassembly, the notes (registers, scratch, LDS and kernarg layout of every kernel) and the .rodata contents.  The raw ELF is not
compared: two compilations of one file differ in their symbol tables.  With several directories (say, a `git worktree` of the
parent commit and this one) the last lines say which sources differ between the first and each other directory.  Needs no GPU.

    python tools/device_digest.py --kernels [csrc directory ...]
hashes per KERNEL instead: each symbol's instruction text without the address column, the raw encoding and the `<symbol+offset>`
branch targets (llvm-objdump prints all three as a trailing comment), and the kernel's own entry in the notes.  One kernel that
changes size moves every address behind it, so the whole-source digest then differs although nothing else does; between two
directories this mode lists exactly the kernels whose code or notes differ, appear or disappear."""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/lib/llvm/bin/"
PER_KERNEL = False


def makefile_vars(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip()  # noqa: E731
    return var("HIPCC"), var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split(), var("SRCS").split()


def digest(csrc, src, hipcc, flags):
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "device.co")  # (the same name everywhere: llvm-objdump prints it)
        subprocess.run([hipcc, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", co], cwd=csrc, check=True,
                       capture_output=True)
        run = lambda *cmd: subprocess.run(cmd, cwd=d, capture_output=True, text=True).stdout  # noqa: E731
        views = (run(LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "device.co"), run(LLVM + "llvm-readelf", "--notes", "device.co"),
                 run(LLVM + "llvm-objdump", "-s", "-j", ".rodata", "device.co"))
    if PER_KERNEL:
        return kernel_digests(views[0], views[1])
    return [hashlib.sha256(v.encode()).hexdigest()[:16] for v in views] + [views[1].count(".sgpr_count")]


def kernel_digests(disassembly, notes):
    """{demangled kernel name: (hash of its instruction text, hash of its entry in the notes)}"""
    sha = lambda text: hashlib.sha256(text.encode()).hexdigest()[:16]  # noqa: E731
    code = {}
    for block in re.split(r"^[0-9a-f]+ <", disassembly, flags=re.M)[1:]:
        name, _, body = block.partition(">:\n")
        code[name] = sha("\n".join(line.split("//")[0].rstrip() for line in body.splitlines()))
    entries = {}
    for entry in re.split(r"^  - (?=\.)", notes.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0], flags=re.M)[1:]:
        entries[re.search(r"\.name:\s+(\S+)", entry).group(1)] = sha(entry)
    names = sorted(entries)
    filt = shutil.which("c++filt") or shutil.which(LLVM + "llvm-cxxfilt")  # (neither: the mangled names)
    plain = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if filt else names
    return {plain[i]: (code[n], entries[n]) for i, n in enumerate(names)}


def digests(csrc):
    hipcc, flags, srcs = makefile_vars(csrc)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(srcs, pool.map(lambda s: digest(csrc, s, hipcc, flags), srcs)))


if __name__ == "__main__":
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-pme_amd", "csrc")
    PER_KERNEL = "--kernels" in sys.argv[1:]
    dirs = [a for a in sys.argv[1:] if a != "--kernels"] or [here]
    results = []
    if PER_KERNEL:
        for k, csrc in enumerate(dirs):
            results.append(digests(csrc))
            print(f"# [{k}] {csrc}: " + "  ".join(f"{src} {len(ks)}" for src, ks in results[-1].items()))
        for k in range(1, len(results)):
            n_same = 0
            for src in sorted(set(results[0]) | set(results[k])):
                a, b = results[0].get(src, {}), results[k].get(src, {})
                n_same += sum(a.get(name) == b.get(name) for name in set(a) & set(b))
                for name in sorted(set(a) | set(b)):
                    if a.get(name) != b.get(name):
                        what = ("only in [0]" if name not in b else f"only in [{k}]" if name not in a else
                                " and ".join(w for w, i in (("code", 0), ("notes", 1)) if a[name][i] != b[name][i]) + " differ")
                        print(f"{src:14s} {what:22s} {name}")
            print(f"# [0] vs [{k}]: {n_same} kernels identical in code and notes")
        sys.exit(0)
    for k, csrc in enumerate(dirs):
        results.append(digests(csrc))
        print(f"# [{k}] {csrc}")
        for src, (dis, notes, rodata, n) in results[-1].items():
            print(f"{src:14s} kernels {n:4d}  disassembly {dis}  notes {notes}  rodata {rodata}")
    for k in range(1, len(results)):
        diff = sorted(s for s in set(results[0]) | set(results[k]) if results[0].get(s) != results[k].get(s))
        print(f"# [0] vs [{k}]: " + ("device code identical for all %d sources" % len(results[0]) if not diff else "DIFFERENT: " + " ".join(diff)))
