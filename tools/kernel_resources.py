#!/usr/bin/env python
"""Resource table of the kernels in a built libkinpoly_sim.so, read from the code objects' metadata (no GPU needed): VGPRs, AGPRs, SGPRs, scratch bytes per
lane, static LDS bytes, code bytes and the registers the allocator spilled (sgpr_spill: scalar registers parked in lanes of a VGPR, vgpr_spill: vector registers
parked in scratch) per kernel.  Two builds of the same sources give identical tables; `--diff other.so` compares them row by row.  `--hash` adds, below
the table, the SHA-256 (first 12 hex digits) of every kernel's code bytes, and `--diff` then compares those too: equal hashes mean the same instructions.

    python tools/kernel_resources.py [lib.so] [--match kp_step_ [--match k_queue_init ...]] [--hash] [--diff other.so]
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ("vgpr", "agpr", "sgpr", "sgpr_spill", "vgpr_spill", "scratch_bytes", "lds_bytes", "code_bytes")


def _llvm(tool: str) -> str:
    for d in (os.path.dirname(shutil.which("hipcc") or ""), "/opt/rocm/bin"):
        p = os.path.normpath(os.path.join(os.path.realpath(d), "..", "lib", "llvm", "bin", tool))
        if os.path.exists(p):
            return p
    for p in (shutil.which(tool), "/opt/rocm/llvm/bin/" + tool):
        if p and os.path.exists(p):
            return p
    raise RuntimeError(f"{tool} not found (ROCm's LLVM tools are required)")


def code_objects(lib: str) -> list[bytes]:
    """the gfx950 ELF images inside the library's .hip_fatbin section (one per translation unit)"""
    with tempfile.TemporaryDirectory() as tmp:
        fb = os.path.join(tmp, "fatbin")
        subprocess.check_call([_llvm("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fb])
        blob = open(fb, "rb").read()
    out = []
    for m in re.finditer(b"\x7fELF\x02\x01", blob):
        o = m.start()
        if struct.unpack_from("<H", blob, o + 18)[0] != 224:           # EM_AMDGPU
            continue
        shoff, = struct.unpack_from("<Q", blob, o + 40)
        shentsize, shnum = struct.unpack_from("<HH", blob, o + 58)
        out.append(blob[o:o + shoff + shentsize * shnum])
    return out


def table(lib: str, hashes: bool = False) -> dict:
    """kernel name (demangled) -> dict of COLS; hashes: also "sha256", the first 12 hex digits over the kernel symbol's bytes in .text"""
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, img in enumerate(code_objects(lib)):
            p = os.path.join(tmp, f"co{i}.o")
            open(p, "wb").write(img)
            notes = subprocess.check_output([_llvm("llvm-readelf"), "--notes", p], text=True)
            sizes, addrs = {}, {}
            for ln in subprocess.check_output([_llvm("llvm-readelf"), "-sW", p], text=True).splitlines():
                f = ln.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    sizes[f[7]] = int(f[2]); addrs[f[7]] = int(f[1], 16)
            if hashes:
                m = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)", subprocess.check_output([_llvm("llvm-readelf"), "-SW", p], text=True))
                text_addr, text_off = int(m.group(1), 16), int(m.group(2), 16)
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                blk = ".agpr_count:" + blk
                g = lambda k: re.search(r"\." + k + r":\s*(\S+)", blk)      # noqa: E731
                sym = g("symbol").group(1)[:-3]                                # drop the .kd suffix
                filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")      # readable names where a demangler exists; the mangled one otherwise
                name = subprocess.check_output([filt, sym], text=True).strip() if filt else sym
                rows[name] = dict(vgpr=int(g("vgpr_count").group(1)), agpr=int(g("agpr_count").group(1)), sgpr=int(g("sgpr_count").group(1)),
                                  sgpr_spill=int(g("sgpr_spill_count").group(1)), vgpr_spill=int(g("vgpr_spill_count").group(1)),
                                  scratch_bytes=int(g("private_segment_fixed_size").group(1)), lds_bytes=int(g("group_segment_fixed_size").group(1)),
                                  code_bytes=sizes.get(sym, -1))
                if hashes:
                    o = addrs[sym] - text_addr + text_off
                    rows[name]["sha256"] = hashlib.sha256(img[o:o + sizes[sym]]).hexdigest()[:12]
    return rows


def render(rows: dict) -> str:
    out = ["| kernel | " + " | ".join(COLS) + " |", "|---|" + "---:|" * len(COLS)]
    for k in sorted(rows):
        out.append(f"| `{k}` | " + " | ".join(str(rows[k][c]) for c in COLS) + " |")
    if any("sha256" in r for r in rows.values()):       # a second table, hash first: parse() reads the one above and skips these rows
        out += ["", "| sha256[:12] of the code | kernel |", "|---|---|"] + [f"| {rows[k]['sha256']} | `{k}` |" for k in sorted(rows)]
    return "\n".join(out)


def parse(md: str) -> dict:
    """a table render() wrote (e.g. a committed profiles/*/kernels_*.md) back as kernel name -> dict of its columns"""
    rows, cols = {}, None
    for ln in md.splitlines():
        f = [c.strip() for c in ln.strip().strip("|").split("|")]
        if ln.startswith("| kernel |"):
            cols = f[1:]
        elif cols and ln.startswith("| `"):
            rows[f[0].strip("`")] = dict(zip(cols, map(int, f[1:])))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib", nargs="?", default=os.path.join(ROOT, "kinpoly_amd", "libkinpoly_sim.so"))
    ap.add_argument("--match", action="append", default=None, help="only kernels whose name contains this; may be given more than once (any of them)")
    ap.add_argument("--diff", default=None, help="another build of the library: exit 1 unless the matched rows are identical")
    ap.add_argument("--hash", action="store_true", help="also the SHA-256 (12 hex digits) of every kernel's code bytes; --diff compares them as well")
    a = ap.parse_args()
    want = lambda k: any(m in k for m in (a.match or [""]))      # noqa: E731
    rows = {k: v for k, v in table(a.lib, a.hash).items() if want(k)}
    print(render(rows))
    if a.diff:
        other = {k: v for k, v in table(a.diff, a.hash).items() if want(k)}
        bad = sorted(k for k in set(rows) | set(other) if rows.get(k) != other.get(k))
        print(f"\n{len(rows)} kernels here, {len(other)} there, {len(bad)} differ" + "".join(f"\n  {k}: {rows.get(k)} != {other.get(k)}" for k in bad))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
