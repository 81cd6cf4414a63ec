"""Digest of the device code of HIP sources: for every kernel of every file, in sorted order, one line

    <file> <kernel symbol> text=<SHA-256 of its instruction text> desc=<SHA-256 of its .amdhsa_kernel block>

The file is compiled with the flags of ``anyloc_amd/build.py`` plus ``--cuda-device-only -S``; the instruction text is the
assembly between the symbol's label and its ``.Lfunc_end``, the descriptor block (registers, LDS, scratch) what stands between
``.amdhsa_kernel`` and ``.end_amdhsa_kernel``.  Comments are dropped and the function's index inside the translation unit
is taken out of its local labels (``.LBB7_3`` -> ``.LBB_3``): the index counts the functions emitted before it, which host
code decides.  Two trees whose outputs are byte-identical ship the same kernels: a host-only change shows as no change here.

    python tools/device_code_digest.py anyloc_amd/csrc/vlad.hip anyloc_amd/csrc/vlad_fused.hip > digest.txt      # no GPU needed
"""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+_(\d+)")


def _sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def _clean(line):
    line = line.split(";", 1)[0].rstrip()
    return LOCAL_LABEL.sub(r".L\1_\2", line)


def digest(path):
    from anyloc_amd import build
    asm = subprocess.run([build.HIPCC] + build.FLAGS + ["--cuda-device-only", "-S", path, "-o", "-"], check=True,
                         stdout=subprocess.PIPE, text=True).stdout.splitlines()
    desc, text = {}, {}
    i = 0
    while i < len(asm):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", asm[i])
        if m:
            j = next(k for k in range(i, len(asm)) if asm[k].strip() == ".end_amdhsa_kernel")
            desc[m.group(1)] = [_clean(x) for x in asm[i + 1:j]]
            i = j
        i += 1
    for name in desc:
        start = asm.index(next(x for x in asm if x.startswith(name + ":")))
        end = next(k for k in range(start, len(asm)) if asm[k].startswith(".Lfunc_end"))
        text[name] = [c for c in (_clean(x) for x in asm[start + 1:end]) if c]
    return [(name, _sha(text[name]), _sha(desc[name])) for name in sorted(desc)]


def main():
    for path in sys.argv[1:]:
        for name, t, d in digest(path):
            print(f"{os.path.basename(path)} {name} text={t} desc={d}")


if __name__ == "__main__":
    main()
