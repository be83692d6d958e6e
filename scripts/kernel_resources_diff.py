"""Compare the kernel descriptors of two source trees.

Compiles the conv / stem / CTR GEMM sources of ``--old`` and ``--new`` (two
``csrc`` directories, e.g. a checkout of the parent commit and the working
tree) to gfx950 assembly and prints, for every kernel name present in both,
the resource fields that differ (VGPRs, SGPRs, LDS bytes, scratch bytes);
then the kernels only the new tree has.  An empty first section means the
change left every existing kernel's register budget alone.

    python scripts/kernel_resources_diff.py --old /tmp/parent/csrc --new csrc
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

FILES = ["conv1x1.hip", "igemm.hip", "halo3x3.hip", "stem.hip", "ctr.hip"]
FIELDS = ["next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def descriptors(csrc: Path, name: str, out: Path) -> dict:
    asm = out / (name + ".s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", f"-I{csrc}",
                    "-munsafe-fp-atomics", "--cuda-device-only", "-S", str(csrc / name), "-o", str(asm)], check=True)
    res, cur = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if ".end_amdhsa_kernel" in line:
            cur = None
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\d+)", line)
        if cur is not None and m and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", required=True, type=Path)
    ap.add_argument("--new", required=True, type=Path)
    ap.add_argument("--jobs", type=int, default=5)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        dirs = {}
        for tag in ("old", "new"):
            dirs[tag] = Path(td) / tag
            dirs[tag].mkdir()
        with cf.ThreadPoolExecutor(a.jobs) as ex:
            futs = {(tag, f): ex.submit(descriptors, getattr(a, tag), f, dirs[tag]) for tag in ("old", "new")
                    for f in FILES}
            res = {k: v.result() for k, v in futs.items()}
    changed = added = common = 0
    for f in FILES:
        old, new = res[("old", f)], res[("new", f)]
        for k in sorted(set(old) & set(new)):
            common += 1
            if old[k] != new[k]:
                changed += 1
                print(f"CHANGED {f} {k}: {old[k]} -> {new[k]}")
        for k in sorted(set(new) - set(old)):
            added += 1
            print(f"NEW {f} {k}: {new[k]}")
        for k in sorted(set(old) - set(new)):
            print(f"GONE {f} {k}")
    print(f"{common} kernels in both trees, {changed} with a changed descriptor, {added} new")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
