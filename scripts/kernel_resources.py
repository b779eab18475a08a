#!/usr/bin/env python3
"""Register / scratch / LDS use of every kernel in a built liblsknn_hip.so, read from the
code-object metadata (no GPU needed):

    python scripts/kernel_resources.py [lib.so] [--match knn_rows] [--json]

One line per kernel: VGPRs, SGPRs, scratch bytes per lane, LDS bytes. Two libraries are
compared by diffing the two outputs (a change that must leave existing kernels alone:
their lines stay identical). Every kernel of the library is listed, e.g. `--match nb_` for the
neighbour-list kernels of knn_neighbors.hip (nb_collect_kernel, nb_ties_kernel, nb_sort_kernel).
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_LIB = os.path.join(ROOT, "mpi_cuda_largescaleknn_amd", "lib", "liblsknn_hip.so")


def _tool(name: str) -> str:
    for cand in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name), shutil.which(name)):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(f"{name} not found (ROCm's llvm/bin)")


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(fat: bytes, arch: str) -> list[bytes]:
    """The `arch` code objects of a .hip_fatbin section: one uncompressed offload bundle per
    translation unit (magic, u64 entry count, then offset / size / triple per entry)."""
    cos, pos = [], fat.find(MAGIC)
    while pos >= 0:
        n = int.from_bytes(fat[pos + 24:pos + 32], "little")
        at = pos + 32
        for _ in range(n):
            off, size, tl = (int.from_bytes(fat[at + 8 * i:at + 8 * i + 8], "little") for i in range(3))
            triple = fat[at + 24:at + 24 + tl].decode()
            at += 24 + tl
            if triple.endswith(arch) and size:
                cos.append(fat[pos + off:pos + off + size])
        pos = fat.find(MAGIC, pos + 1)
    return cos


def kernel_resources(lib: str, arch: str = "gfx950") -> dict[str, dict[str, int]]:
    notes = ""
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.run([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        with open(fat, "rb") as f:
            blobs = _code_objects(f.read(), arch)
        for i, blob in enumerate(blobs):
            co = os.path.join(tmp, f"code{i}.co")
            with open(co, "wb") as f:
                f.write(blob)
            notes += subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, stdout=subprocess.PIPE,
                                    text=True).stdout
    out: dict[str, dict[str, int]] = {}
    fields = {".vgpr_count": "vgpr", ".sgpr_count": "sgpr", ".private_segment_fixed_size": "scratch",
              ".group_segment_fixed_size": "lds"}
    # the kernels' metadata: YAML blocks "- .agpr_count: ..." with one ".name:" each
    for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\n\s*\.name:\s*(\S+)", block)
        if not name:
            continue
        vals = {}
        for key, short in fields.items():
            m = re.search(r"\n\s*" + re.escape(key) + r":\s*(\d+)", block)
            vals[short] = int(m.group(1)) if m else -1
        out[name.group(1)] = vals
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default=DEFAULT_LIB)
    ap.add_argument("--match", default="", help="only kernels whose (mangled) name contains this")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    res = {k: v for k, v in kernel_resources(a.lib).items() if a.match in k}
    if a.json:
        print(json.dumps(res, indent=1, sort_keys=True))
    else:
        for k in sorted(res):
            v = res[k]
            print(f"{k}  vgpr {v['vgpr']}  sgpr {v['sgpr']}  scratch {v['scratch']}  lds {v['lds']}")
    return 0 if res else 1


if __name__ == "__main__":
    sys.exit(main())
