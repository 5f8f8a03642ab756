#!/usr/bin/env python3
"""Compare the device code of the GEMM translation units at two revisions.

    scripts/gemm_isa_diff.py [REV_A [REV_B]]     (CPU only; needs hipcc)

REV_A defaults to HEAD; REV_B defaults to the working tree. For each side
hpc_patterns_amd/native is exported to a temporary directory and every
gemm*.hip in it is compiled device-only to assembly with the Makefile's
flags. Per kernel the script prints the instruction count, VGPRs, AGPRs, LDS
bytes, scratch bytes, waves/SIMD and whether the two instruction streams are
identical once block labels, mangled symbols and the __hip_cuid_<hash> lines
are normalised. It exits 1 if any kernel differs, was added or was removed.

This is rung A of profiles/gemm_refactor_ab.md: a refactor of these files
ships only where the kernels that exist keep their code
(docs/findings.md #28). It only compares; it looks for no instruction.
"""

from __future__ import annotations

import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile
from dataclasses import dataclass, field
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
NATIVE = "hpc_patterns_amd/native"

_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")
_MANGLED = re.compile(r"_Z\w+")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_RESOURCE = re.compile(
    r";\s*(NumVgprs|NumAgprs|ScratchSize|LDSByteSize|Occupancy):\s*(\d+)")


def normalise(body: str) -> list[str]:
    """The instruction stream of one function's assembly text, made
    comparable: comments, directives and blank lines dropped, white space
    collapsed, block labels renamed L0, L1, ... and mangled symbols S0, S1,
    ... in order of first appearance, the hash of __hip_cuid_<hash> dropped.
    Instructions, their order, operands and register numbers are kept."""
    names: dict[str, str] = {}

    def rename(prefix: str):
        def sub(m: re.Match) -> str:
            return names.setdefault(
                m.group(0),
                f"{prefix}{sum(v.startswith(prefix) for v in names.values())}")
        return sub

    out = []
    for line in body.splitlines():
        line = " ".join(line.split(";", 1)[0].split())
        if not line:
            continue
        if line.startswith(".") and not line.endswith(":"):
            continue  # directive; a block label ends in ':'
        line = _CUID.sub("__hip_cuid_", line)
        line = _LABEL.sub(rename("L"), line)
        line = _MANGLED.sub(rename("S"), line)
        out.append(line)
    return out


@dataclass
class Kernel:
    stream: list[str] = field(default_factory=list)
    resources: dict[str, int] = field(default_factory=dict)

    @property
    def instructions(self) -> int:
        return sum(not s.endswith(":") for s in self.stream)


def split_kernels(asm: str) -> dict[str, Kernel]:
    """Mangled name -> Kernel for every function of a device assembly file.
    A function runs from `name:` behind its `.type name,@function` to its
    .Lfunc_end label; the resource comments that follow belong to it."""
    kernels: dict[str, Kernel] = {}
    name, body, last = None, [], None
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            name, body = m.group(1), None
            continue
        if name and body is None:
            if s.startswith(name + ":"):
                body = []
            continue
        if name and s.startswith(".Lfunc_end"):
            kernels[name] = last = Kernel(normalise("\n".join(body)))
            name = None
            continue
        if name:
            body.append(line)
        elif last is not None:
            r = _RESOURCE.search(s)
            if r:
                last.resources.setdefault(r.group(1), int(r.group(2)))
    return kernels


def compare(asm_a: str, asm_b: str) -> list[tuple[str, Kernel | None,
                                                  Kernel | None, str]]:
    """(name, kernel in A, kernel in B, verdict) per kernel of either file,
    A's order first. Verdicts: identical, different, added, removed."""
    a, b = split_kernels(asm_a), split_kernels(asm_b)
    rows = []
    for name in list(a) + [n for n in b if n not in a]:
        ka, kb = a.get(name), b.get(name)
        if ka is None:
            verdict = "added"
        elif kb is None:
            verdict = "removed"
        elif ka.stream == kb.stream and ka.resources == kb.resources:
            verdict = "identical"
        else:
            verdict = "different"
        rows.append((name, ka, kb, verdict))
    return rows


def makefile_flags() -> list[str]:
    text = (ROOT / "Makefile").read_text()
    arch = re.search(r"^GPU_ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(GPU_ARCH)", arch).replace("$(NATIVE)", ".")
    return flags.split()


def export(rev: str | None, dest: Path) -> Path:
    if rev is None:
        shutil.copytree(ROOT / NATIVE, dest / NATIVE)
    else:
        tar = subprocess.run(["git", "-C", str(ROOT), "archive", rev, NATIVE],
                             check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", str(dest)], input=tar, check=True)
    return dest / NATIVE


def assemble(native: Path, hipcc: str, flags: list[str]) -> dict[str, str]:
    def one(src: Path) -> tuple[str, str]:
        out = src.with_suffix(".s")
        res = subprocess.run(
            [hipcc, *flags, "--cuda-device-only", "-S", src.name, "-o",
             out.name], cwd=native, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError(f"{src}: {res.stderr[-2000:]}")
        return src.name, out.read_text()

    srcs = sorted(native.glob("gemm*.hip"))
    jobs = min(8, os.cpu_count() or 1)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        return dict(pool.map(one, srcs))


def demangle(names: list[str]) -> dict[str, str]:
    tool = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or \
        shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), text=True,
                         capture_output=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = d.replace("hpk::(anonymous namespace)::", "")
        d = re.sub(r"^void ", "", d)
        if d.endswith(")"):  # drop the argument list: name<...> is enough
            depth, i = 0, len(d)
            while i > 0:
                i -= 1
                depth += (d[i] == ")") - (d[i] == "(")
                if depth == 0:
                    break
            d = d[:i]
        short[n] = d
    return short


def pair(ka: Kernel | None, kb: Kernel | None, get) -> str:
    return " / ".join("-" if k is None else str(get(k)) for k in (ka, kb))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev_a", nargs="?", default="HEAD")
    ap.add_argument("rev_b", nargs="?", default=None,
                    help="default: the working tree")
    ap.add_argument("--hipcc", default=os.environ.get(
        "HIPCC", "/opt/rocm/bin/hipcc"))
    args = ap.parse_args()

    flags = makefile_flags()
    with tempfile.TemporaryDirectory() as ta, \
            tempfile.TemporaryDirectory() as tb:
        asm_a = assemble(export(args.rev_a, Path(ta)), args.hipcc, flags)
        asm_b = assemble(export(args.rev_b, Path(tb)), args.hipcc, flags)

    print(f"A = {args.rev_a}, B = {args.rev_b or 'working tree'}; "
          f"hipcc {' '.join(flags)} --cuda-device-only -S; every column A / B")
    bad = 0
    for fname in sorted(set(asm_a) | set(asm_b)):
        rows = compare(asm_a.get(fname, ""), asm_b.get(fname, ""))
        names = demangle([r[0] for r in rows])
        print(f"\n### {fname}: {len(rows)} kernels\n")
        print("| kernel | instr | VGPR | AGPR | LDS bytes | scratch | "
              "waves/SIMD | streams |")
        print("|---|---|---|---|---|---|---|---|")
        for name, ka, kb, verdict in rows:
            bad += verdict != "identical"
            cols = [pair(ka, kb, lambda k: k.instructions)]
            for key in ("NumVgprs", "NumAgprs", "LDSByteSize", "ScratchSize",
                        "Occupancy"):
                cols.append(pair(ka, kb, lambda k: k.resources.get(key, "?")))
            print(f"| `{names[name]}` | " + " | ".join(cols) +
                  f" | {verdict} |")
    print(f"\n{bad} kernel(s) not identical" if bad else
          "\nevery kernel identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
