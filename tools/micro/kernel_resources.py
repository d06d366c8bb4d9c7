"""usage (no GPU needed): python tools/micro/kernel_resources.py [--csrc DIR] file.hip ... > table.txt
One line per kernel of the given files, compiled with the command `make -n` prints for the file: VGPRs, AGPRs, LDS bytes,
scratch bytes per lane and waves per SIMD from -Rpass-analysis=kernel-resource-usage, the number of MFMA and global_load_lds
instructions in the -S output,
and a digest of the kernel's inline-asm statements (what -S brackets with #ASMSTART / #ASMEND; register numbers masked).  The
statements themselves follow per file, each with the number of kernels * occurrences.  Two such tables are compared with
`diff`: see profiles/gemm_refactor_resources.txt."""
import collections
import hashlib
import os
import re
import shlex
import subprocess
import sys
import tempfile

KEYS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("LDS Size [bytes/block]", "LDS"), ("ScratchSize [bytes/lane]", "scratch"),
        ("Occupancy [waves/SIMD]", "occ"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, out))


def table(csrc, f):
    # the Makefile's own command line for this file (per-file MFMA form and extra flags included), compiled for the device only
    rule = subprocess.run(["make", "-n", "-B", "build/" + f.replace(".hip", ".o")], cwd=csrc, capture_output=True, text=True, check=True).stdout
    cmd = shlex.split(next(l for l in rule.splitlines() if " -c " in l))
    cmd = cmd[:cmd.index("-c")] + ["-Rpass-analysis=kernel-resource-usage", "--offload-device-only", "-S", f, "-o"]
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "k.s")
        cmd.append(s)
        err = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True, check=True).stderr
        asm = open(s).read()
    res, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([^:]+): (\d+))", line)
        if m and m.group(1):
            cur = res.setdefault(m.group(1), {})
        elif m and cur is not None:
            cur[m.group(2).strip()] = int(m.group(3))
    counts = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end", asm, re.M | re.S):
        body = m.group(2)
        stmts = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", " | ".join(t.strip() for t in b.strip().splitlines()))
                 for b in re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", body, re.S)]
        counts[m.group(1)] = (len(re.findall(r"^\s+v_mfma_", body, re.M)), len(re.findall(r"^\s+global_load_lds_", body, re.M)),
                              collections.Counter(stmts))
    names = demangle(sorted(res))
    rows, stmts_all = [], collections.Counter()
    for k in sorted(res, key=lambda k: names[k]):
        if k not in counts:
            continue        # a device function, not a kernel body of this file's -S output
        mfma, dma, st = counts[k]
        digest = hashlib.sha1("\n".join(f"{n} {s}" for s, n in sorted(st.items())).encode()).hexdigest()[:8]
        stmts_all.update(st)
        cols = " ".join(f"{short} {res[k].get(key, 0)}" for key, short in KEYS)
        rows.append(f"{f} {names[k]} : {cols} mfma {mfma} dma {dma} asm {sum(st.values())}/{digest}")
    rows += [f"{f} asm x{n}: {s}" for s, n in sorted(stmts_all.items())]
    return rows


if __name__ == "__main__":
    args = sys.argv[1:]
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "demucs_amd", "csrc")
    if args[:1] == ["--csrc"]:
        csrc, args = args[1], args[2:]
    for f in args:
        print("\n".join(table(csrc, f)))
