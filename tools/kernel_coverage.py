"""Which compiled kernel instantiations does a test ever launch?

    python tools/kernel_coverage.py compiled                      # the kernel instantiations of the built library (no GPU)
    python tools/kernel_coverage.py launched DIR...               # the same names from rocprofv3 --kernel-trace CSV files
    python tools/kernel_coverage.py report DIR... [--tsv FILE]    # per compiled kernel: the traces that launched it, or NEVER

``compiled`` reads the device code of every object under anyloc_amd/build/ (llvm-objcopy copies the .hip_fatbin section out,
clang-offload-bundler unbundles the gfx950 code object, llvm-readelf lists its symbols, c++filt demangles the kernel descriptors
``*.kd``) and prints one line per kernel, ``<name>\t<source file>``, and the count.  Where the objects are gone but the library
is there, the library's own .hip_fatbin section (one bundle per source file) gives the same names without their source files.

A name is normalised to ``kernel<template arguments>``: no return type, no ``anyloc::``, no ``(anonymous namespace)::``, no
parameter list, no ``.kd``.  The same function normalises the names of a kernel trace, so the two sides compare as strings.

``launched`` takes directories of ``rocprofv3 --kernel-trace --output-format csv`` runs (read by tools/kernel_trace_launches.py),
one directory per traced test file: the directory's last path component is the witness the report names.  In place of a
directory it also takes a file holding what an earlier ``launched`` printed, so that the traces of a large suite can be reduced
where they were taken and joined later.  It prints
``<name>\t<launches>\t<witnesses>`` and exits non-zero if a traced kernel whose name contains ``anyloc::`` is not in the
compiled list -- the check that normalisation works on both sides.

``report`` joins the two: per compiled kernel the witnesses or ``NEVER``, then totals per source file.  ``--tsv`` writes the
rows in the format of tests/kernel_coverage.tsv (kernels of the two exempt families that no trace launched become ``exempt``
rows; any other NEVER kernel is written as ``test`` with the witness ``NEVER``, which tests/test_kernel_coverage_cpu.py
refuses).  ``--merge TABLE`` adds the witnesses of an earlier table to those of the traces: after a change, trace the test
files that changed and merge the rest.  DESIGN.md ("Kernel launch coverage") has the recipe of the audit run."""
import argparse
import collections
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "anyloc_amd", "build")
LIB = os.path.join(ROOT, "anyloc_amd", "libanyloc_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")

# the two families that cannot be held to a reference (include/anyloc_hip.h: gemm_f32_cfg 5 - 8 "compute wrong results", timing
# only; csrc/vlad_fused.hip: vlad_gather_v != 0 "not reproducible run to run") have at most this many kernels: exempt_reason
EXEMPT_MAX = 14


def _args(name):
    """'kernel<a, b<c, d>, e>' -> ('kernel', ['a', 'b<c, d>', 'e'])"""
    if "<" not in name:
        return name, []
    base, rest = name.split("<", 1)
    rest, out, depth, cur = rest[:rest.rindex(">")], [], 0, ""
    for ch in rest:
        if ch == "," and depth == 0:
            out.append(cur.strip()); cur = ""
            continue
        depth += ch in "<(" ; depth -= ch in ">)"
        cur += ch
    return base, out + [cur.strip()]


def exempt_reason(name):
    """The documented reason a kernel has no parity test, or None: only the two study families qualify."""
    base, a = _args(name)
    if base == "gemm_nt_kernel" and a and a[-1] in ("1", "2", "3", "4"):
        return f"gemm_f32_cfg {4 + int(a[-1])}: timing-only ablation {a[-1]}, documented in include/anyloc_hip.h as computing wrong results"
    if base == "fused3_kernel" and a and a[-1] not in ("0", "false"):
        return "vlad_gather_v != 0: hazard study variant, documented in csrc/vlad_fused.hip as not reproducible run to run"
    return None


def _rocm_tool(name):
    for d in (os.environ.get("ROCM_LLVM_BIN"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"),
              os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")):
        if d and os.path.isfile(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def tools_missing():
    """the names of the binaries ``compiled`` needs and this host lacks"""
    need = ["llvm-objcopy", "clang-offload-bundler", "llvm-readelf"]
    missing = [n for n in need if not _rocm_tool(n)]
    if not (shutil.which("c++filt") or _rocm_tool("llvm-cxxfilt")):
        missing.append("c++filt")
    return missing


_INT_SUFFIX = re.compile(r"(?<![\w.])(\d+)(?:ul{0,2}|l{1,2})\b", re.I)
_CAST = re.compile(r"\((?:unsigned |signed )?(?:bool|char|short|int|long|long long|[\w:]+)\)(?=-?\d)")


def normalise(demangled):
    """'void anyloc::(anonymous namespace)::k<2, (bool)1>(float*, int) [clone .kd]' -> 'k<2, true>'"""
    s = demangled.strip()
    s = re.sub(r"\s*\[clone \.kd\]$|\.kd$|\s*\(\.kd\)$", "", s)
    s = s.replace("(anonymous namespace)::", "").replace("'anonymous namespace'::", "").replace("anyloc::", "")
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):                            # the parameter list: the first '(' outside every '<...>'
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut].strip()
    depth, start = 0, 0
    for i, ch in enumerate(s):                            # the return type: up to the last blank outside every '<...>'
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == " " and depth == 0:
            start = i + 1
    s = s[start:]
    # demanglers differ in how they print a non-type argument: (bool)1 / true, 3u / 3, (anyloc::Kind)3 / 3
    s = s.replace("(bool)1", "true").replace("(bool)0", "false")
    s = _CAST.sub("", s)
    s = _INT_SUFFIX.sub(r"\1", s)
    base, a = _args(s)
    return f"{base}<{', '.join(a)}>" if a else base


def _run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw).stdout


def _kd_names(fatbin_bytes, tmp):
    """normalised kernel names of the gfx950 code object of ONE offload bundle"""
    fb, co = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.co")
    with open(fb, "wb") as f:
        f.write(fatbin_bytes)
    _run([_rocm_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fb}", f"--output={co}"])
    syms = set()
    for line in _run([_rocm_tool("llvm-readelf"), "-sW", co]).decode().splitlines():
        f = line.split()
        if f and f[-1].endswith(".kd"):
            syms.add(f[-1][:-3])
    if not syms:
        return set()
    filt = shutil.which("c++filt") or _rocm_tool("llvm-cxxfilt")
    out = _run([filt], input="\n".join(sorted(syms)).encode()).decode().splitlines()
    return {normalise(n) for n in out}


def _bundles(path, tmp):
    """the offload bundles in the .hip_fatbin section of an object (one) or of the linked library (one per source file)"""
    sec = os.path.join(tmp, "section.bin")
    _run([_rocm_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, sec])
    with open(sec, "rb") as f:
        data = f.read()
    starts = sorted({m.start() for magic in BUNDLE_MAGIC for m in re.finditer(re.escape(magic), data) if m.start() % 4096 == 0})
    return [data[a:b] for a, b in zip(starts, starts[1:] + [len(data)])]


def compiled():
    """{normalised kernel name: source file ('?' when read from the linked library)} of the built library"""
    missing = tools_missing()
    if missing:
        raise RuntimeError("missing ROCm binaries: " + ", ".join(missing))
    objs = sorted(glob.glob(os.path.join(OBJ, "*.o")))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        if objs:
            for o in objs:
                src = os.path.basename(o)[:-2] + ".hip"
                for b in _bundles(o, tmp):
                    for n in _kd_names(b, tmp):
                        assert out.setdefault(n, src) == src, f"{n} is compiled in {out[n]} and in {src}: the names no longer tell kernels apart"
        elif os.path.isfile(LIB):
            for b in _bundles(LIB, tmp):
                for n in _kd_names(b, tmp):
                    out.setdefault(n, "?")
        else:
            raise RuntimeError(f"nothing built: neither {OBJ}/*.o nor {LIB} (python -m anyloc_amd.build)")
    return out


def launched(dirs):
    """{normalised name: {witness: launches}} of the anyloc kernels in the traces, and the raw names that are not normalised ones
    of the compiled list"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from kernel_trace_launches import launches
    have = compiled()
    seen, unmatched = collections.defaultdict(collections.Counter), set()
    for d in dirs:
        if os.path.isfile(d) and not d.endswith(".csv"):  # the listing an earlier ``launched`` printed
            with open(d) as f:
                for line in f:
                    if line.strip() and not line.startswith("#"):
                        n, _, wit = line.rstrip("\n").split("\t")
                        for w in wit.split(","):
                            seen[n][w.rsplit(":", 1)[0]] += int(w.rsplit(":", 1)[1])
                        if n not in have:
                            unmatched.add(n)
            continue
        witness = os.path.basename(os.path.normpath(d))
        for line in launches(d, "anyloc::"):
            raw = line[:line.rindex(" grid=")]
            n = normalise(raw)
            seen[n][witness] += 1
            if n not in have:
                unmatched.add(raw)
    return seen, unmatched, have


def tsv_rows(have, seen):
    rows = []
    for n in sorted(have):
        if n in seen:
            rows.append((n, have[n], "test", ",".join(sorted(seen[n]))))
        elif exempt_reason(n):
            rows.append((n, have[n], "exempt", exempt_reason(n)))
        else:
            rows.append((n, have[n], "test", "NEVER"))
    return rows


def read_tsv(path):
    with open(path) as f:
        return [tuple(l.rstrip("\n").split("\t")) for l in f if l.strip() and not l.startswith("#")]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("compiled")
    for name in ("launched", "report"):
        p = sub.add_parser(name)
        p.add_argument("dirs", nargs="+", help="one rocprofv3 output directory per traced test file, or a file with the output of an earlier 'launched'")
        if name == "report":
            p.add_argument("--tsv", help="write the rows of tests/kernel_coverage.tsv here")
            p.add_argument("--merge", help="an earlier table: its witnesses are added to those of the traces")
    args = ap.parse_args()
    if args.cmd == "compiled":
        have = compiled()
        for n in sorted(have):
            print(f"{n}\t{have[n]}")
        per = collections.Counter(have.values())
        for src, c in per.most_common():
            print(f"# {src}\t{c}")
        print(len(have))
        return 0
    seen, unmatched, have = launched(args.dirs)
    for raw in sorted(unmatched):
        print(f"NOT IN THE COMPILED LIST: {raw}", file=sys.stderr)
    if args.cmd == "launched":
        for n in sorted(seen):
            print(f"{n}\t{sum(seen[n].values())}\t{','.join(f'{w}:{c}' for w, c in sorted(seen[n].items()))}")
        print(f"# {len(seen)} kernels, {sum(sum(c.values()) for c in seen.values())} launches, {len(unmatched)} unmatched")
        return 1 if unmatched else 0
    if args.merge:
        for n, _, kind, wit in read_tsv(args.merge):
            if kind == "test" and wit != "NEVER":
                for w in wit.split(","):
                    seen[n][w] += 0
    rows = tsv_rows(have, seen)
    per = collections.defaultdict(lambda: [0, 0, 0])
    for n, src, kind, wit in rows:
        print(f"{n}\t{src}\t{'EXEMPT' if kind == 'exempt' else wit}")
        per[src][0] += 1
        per[src][1] += kind == "test" and wit != "NEVER"
        per[src][2] += kind == "exempt"
    print("# source\tcompiled\tlaunched\texempt\tNEVER")
    tot = [0, 0, 0]
    for src in sorted(per, key=lambda s: -per[s][0]):
        c, l, e = per[src]
        tot = [tot[0] + c, tot[1] + l, tot[2] + e]
        print(f"# {src}\t{c}\t{l}\t{e}\t{c - l - e}")
    print(f"# total\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[0] - tot[1] - tot[2]}")
    if args.tsv:
        with open(args.tsv, "w") as f:
            f.write("# kernel\tsource\ttest|exempt\tthe test files that launch it (audit: tools/kernel_coverage.py report) | why it is exempt\n")
            for r in rows:
                f.write("\t".join(r) + "\n")
    return 1 if unmatched else 0


if __name__ == "__main__":
    sys.exit(main())
