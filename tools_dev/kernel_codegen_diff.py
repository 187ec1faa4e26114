#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two versions of occnet_amd/csrc (CPU only, no GPU involved).

    python tools_dev/kernel_codegen_diff.py BASE NEW [--jobs 8] [--keep DIR]

BASE / NEW: a csrc directory (its *.hip are compiled to device assembly with the library's own flags from the
build.py next to it, plus --cuda-device-only -S) or a directory of *.s files from such a run.

For a refactor that must not change what a kernel computes or how fast it runs, per kernel:
  * the same kernel names;
  * identical .vgpr_count, .sgpr_count, .private_segment_fixed_size, .group_segment_fixed_size;
  * identical instruction-mnemonic histograms, except that s_nop and s_waitcnt counts may move.
Per file it also says whether the text is byte-identical once .file / .loc / .ident and comments are dropped.
Exit status 1 when any kernel is outside that bar.
"""
import argparse
import collections
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

META = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
FREE = ("s_nop", "s_waitcnt")


def build_flags(csrc):
    spec = importlib.util.spec_from_file_location("_occ_build", os.path.join(csrc, "..", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.hipcc(), mod.FLAGS


def assemble(csrc, out, jobs):
    hipcc, flags = build_flags(csrc)
    os.makedirs(out, exist_ok=True)

    def one(name):
        dst = os.path.join(out, name[:-4] + ".s")
        cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-o", dst, os.path.join(csrc, name)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            sys.exit(f"hipcc failed on {csrc}/{name}\n{res.stderr}")

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        list(ex.map(one, sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))))
    return out


def normalised(text):
    """The assembly without debug directives, comments, blank lines and the per-compilation __hip_cuid_ symbol."""
    keep = []
    for line in text.splitlines():
        line = line.split(";", 1)[0].rstrip()
        if line and not re.match(r"\s*\.(file|loc|ident)\b", line) and "__hip_cuid_" not in line:
            keep.append(line)
    return keep


def kernels(text):
    """{kernel name: (metadata dict, mnemonic Counter)} of one .s file."""
    meta = {}
    block = text[text.find("amdhsa.kernels:"):text.find(".end_amdgpu_metadata")]
    for rec in re.split(r"^  - ", block, flags=re.M)[1:]:          # one record per kernel, its own keys indented by 4
        keys = dict(re.findall(r"^(?:    )?(\.\w+):\s+(\S+)$", rec, flags=re.M))
        if ".name" in keys:                                         # (the version list that follows has none)
            meta[keys[".name"]] = {k: keys.get(k) for k in META}
    out, body, name = {}, None, None
    for line in text.splitlines():
        m = re.match(r"(\w+):", line)
        if m and m.group(1) in meta:
            name, body = m.group(1), collections.Counter()
        elif name and line.startswith(".Lfunc_end"):
            out[name] = (meta[name], body)
            name = None
        elif name and line.startswith("\t") and not line.startswith(("\t.", "\t;")):
            body[line.split()[0]] += 1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="write the assembly under DIR/base and DIR/new instead of a temporary directory")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="codegen_diff_")
    dirs = []
    for tag, d in (("base", args.base), ("new", args.new)):
        has_hip = any(f.endswith(".hip") for f in os.listdir(d))
        dirs.append(assemble(d, os.path.join(tmp, tag), args.jobs) if has_hip else d)
    files = [sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in dirs]
    bad = n_base = n_new = 0
    for f in sorted(set(files[0]) | set(files[1])):
        if f not in files[0] or f not in files[1]:
            print(f"{f}: only in {'base' if f in files[0] else 'new'}")
            bad += 1
            continue
        a, b = (open(os.path.join(d, f)).read() for d in dirs)
        ka, kb = kernels(a), kernels(b)
        n_base += len(ka)
        n_new += len(kb)
        if normalised(a) == normalised(b):
            print(f"{f}: identical ({len(ka)} kernels)")
            continue
        notes = []
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                notes.append((k, f"only in {'base' if k in ka else 'new'}", False))
                continue
            (ma, ha), (mb, hb) = ka[k], kb[k]
            dm = [f"{x} {ma.get(x)} -> {mb.get(x)}" for x in META if ma.get(x) != mb.get(x)]
            dh = [f"{x} {ha[x]} -> {hb[x]}" for x in sorted(set(ha) | set(hb)) if ha[x] != hb[x]]
            ok = not dm and all(x.split()[0] in FREE for x in dh)
            if dm or dh:
                notes.append((k, "; ".join(dm + dh), ok))
        within = sum(ok for _, _, ok in notes)
        print(f"{f}: text differs; {len(ka) - len(notes)} of {len(ka)} kernels with equal resources and histograms, "
              f"{within} differ in s_nop / s_waitcnt only, {len(notes) - within} OUTSIDE the bar")
        for k, what, ok in notes:
            print(f"    {'ok ' if ok else 'BAD'} {k}: {what}")
            bad += not ok
    if not args.keep:
        shutil.rmtree(tmp)
    print(f"kernels: base {n_base}, new {n_new}; outside the bar: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
