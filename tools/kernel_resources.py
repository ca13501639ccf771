#!/usr/bin/env python3
"""Register, LDS and occupancy report of kernels (CPU only).

Compiles the sources device-only with the Makefile's flags plus
-Rpass-analysis=kernel-resource-usage and prints, as JSON, the VGPRs, SGPRs,
spilled SGPRs / VGPRs, scratch bytes, LDS bytes and waves per SIMD of every
instance of the kernels, followed by a diff against the "head" entry of a
record file (the fields that the record holds).  By default: skge_pipeline.hip
and skge_hole_pipe.hip, every k_pipe_batch, k_pipe_fused and k_hole_pipe
instance, against profiles/pipe_regression/resources.json.  It reads the
compiler's remarks only; nothing runs on a GPU.

Usage: tools/kernel_resources.py [--csrc DIR] [--sources A.hip,B.hip] [--kernels K1,K2]
                                 [--record FILE] [--write FILE] [-- extra hipcc flags]
  --csrc DIR     another tree's csrc/ (e.g. an exported revision)
  --sources ...  the files of csrc/ to compile
  --kernels ...  the kernel names (without template arguments) to report
  --record FILE  the record to diff against
  --write FILE   also write the report to FILE
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "scikit-kge_amd")
RECORD = os.path.join(ROOT, "profiles", "pipe_regression", "resources.json")
SOURCES = ("skge_pipeline.hip", "skge_hole_pipe.hip")
KERNELS = ("k_pipe_batch", "k_pipe_fused", "k_hole_pipe")
FIELDS = {"SGPRs": "sgprs", "TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes",
          "Occupancy [waves/SIMD]": "waves_per_simd", "SGPRs Spill": "sgpr_spills",
          "VGPRs Spill": "vgpr_spills", "LDS Size [bytes/block]": "lds_bytes"}


def makefile_flags():
    """HIPCC, and CXXFLAGS with $(ARCH) expanded, as the Makefile states them."""
    var = {}
    for line in open(os.path.join(PKG, "Makefile")):
        m = re.match(r"^(\w+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m:
            var[m.group(1)] = m.group(2)
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["CXXFLAGS"])
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def demangle(names, hipcc):
    filt = os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def remarks(src, hipcc, flags, extra):
    cmd = [hipcc] + flags + list(extra) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                                           "-c", src, "-o", os.devnull]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.stderr.write(p.stderr)
        raise SystemExit("kernel_resources: %s did not compile" % src)
    out, cur = {}, None
    for line in p.stderr.split("\n"):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z][^:]*): (\S+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def report(csrc, extra=(), sources=SOURCES, kernels=KERNELS):
    hipcc, flags = makefile_flags()
    res = {}
    for s in sources:
        path = os.path.join(csrc, s)
        if not os.path.exists(path):
            continue
        rm = remarks(path, hipcc, flags, extra)
        names = demangle(list(rm), hipcc)
        for mangled, r in rm.items():
            name = names[mangled]
            m = re.match(r"^(?:void )?skge::(\w+)(<.*>)?\(", name)
            if m and m.group(1) in kernels:
                res[m.group(1) + (m.group(2) or "")] = r
    return dict(sorted(res.items()))


def diff(new, old):
    out = {}
    for k in sorted(set(new) | set(old)):
        if k not in old:
            out[k] = "new"
        elif k not in new:
            out[k] = "gone"
        else:
            ch = {f: [old[k][f], new[k].get(f)] for f in FIELDS.values()
                  if f in old[k] and old[k][f] != new[k].get(f)}
            if ch:
                out[k] = ch
    return out


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(PKG, "csrc"))
    ap.add_argument("--sources", default=",".join(SOURCES))
    ap.add_argument("--kernels", default=",".join(KERNELS))
    ap.add_argument("--record", default=RECORD)
    ap.add_argument("--write", default=None)
    args = ap.parse_args(argv)
    res = report(args.csrc, extra, args.sources.split(","), args.kernels.split(","))
    out = {"resources": res}
    if os.path.exists(args.record):
        rec = json.load(open(args.record))
        out["diff_against_record"] = diff(res, rec.get("head", {}))   # [recorded, now]
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.write:
        with open(args.write, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
