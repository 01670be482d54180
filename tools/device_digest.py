"""Digest of the DEVICE code of every .hip source of libmipme, to show that a host-side change left the kernels alone:
    python tools/device_digest.py [csrc directory ...]        (default: torch-pme_amd/csrc of this checkout)
Each source is compiled for the device only, with the Makefile's flags, and three views of the code object are hashed: the
disassembly, the notes (registers, scratch, LDS and kernarg layout of every kernel) and the .rodata contents.  The raw ELF is not
compared: two compilations of one file differ in their symbol tables.  With several directories (say, a `git worktree` of the
parent commit and this one) the last lines say which sources differ between the first and each other directory.  Needs no GPU."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/lib/llvm/bin/"


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
    return [hashlib.sha256(v.encode()).hexdigest()[:16] for v in views] + [views[1].count(".sgpr_count")]


def digests(csrc):
    hipcc, flags, srcs = makefile_vars(csrc)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return dict(zip(srcs, pool.map(lambda s: digest(csrc, s, hipcc, flags), srcs)))


if __name__ == "__main__":
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torch-pme_amd", "csrc")
    dirs = sys.argv[1:] or [here]
    results = []
    for k, csrc in enumerate(dirs):
        results.append(digests(csrc))
        print(f"# [{k}] {csrc}")
        for src, (dis, notes, rodata, n) in results[-1].items():
            print(f"{src:14s} kernels {n:4d}  disassembly {dis}  notes {notes}  rodata {rodata}")
    for k in range(1, len(results)):
        diff = sorted(s for s in set(results[0]) | set(results[k]) if results[0].get(s) != results[k].get(s))
        print(f"# [0] vs [{k}]: " + ("device code identical for all %d sources" % len(results[0]) if not diff else "DIFFERENT: " + " ".join(diff)))
