#!/usr/bin/env python3
"""Fingerprint every gfx950 kernel of the device library, to prove a refactor.

  tools/kernel_fingerprint.py [--tree DIR] [--source FILE.hip ...] [-o OUT.json]
      compiles each source of DIR's csrc/build.py with that build's flags plus
      ``--cuda-device-only --no-gpu-bundle-output -c`` (no GPU needed, at most 8 compiles
      at a time) and prints, per kernel symbol, the demangled name, the sha256 of its
      machine-code bytes and the sha256 of its 64-byte ``.kd`` descriptor.
  tools/kernel_fingerprint.py --diff OLD.json NEW.json [--rename 'OLD=>NEW' ...]
      lists the kernels only in OLD, only in NEW, and changed; exit status 1 if any.
      ``--rename`` rewrites OLD's names by a regular expression before comparing (a
      template parameter that went away).

Bytes are hashed, not text, so the result does not depend on the ``__hip_cuid_*`` symbol or
on ``.LBB<n>_`` label numbers.  The one position-dependent field of the descriptor, the
8-byte kernel_code_entry_byte_offset at byte 16 (the distance from the descriptor to the
code, which moves with every neighbour), is hashed as zero.  The tool only hashes; it
inspects no instructions.
"""
from __future__ import annotations

import argparse
import hashlib
import importlib.util
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_ENTRY_OFFSET = slice(16, 24)  # kernel_code_entry_byte_offset


def elf_kernels(path: str) -> dict:
    """{mangled name: (code bytes, descriptor bytes)} of an AMDGPU code object: every
    ``NAME.kd`` object symbol of 64 bytes together with the function symbol ``NAME``."""
    with open(path, "rb") as f:
        b = f.read()
    if b[:6] != b"\x7fELF\x02\x01":
        raise ValueError(f"{path}: not a little-endian ELF64 file")
    e_type, = struct.unpack_from("<H", b, 16)
    e_shoff, = struct.unpack_from("<Q", b, 40)
    e_shentsize, e_shnum = struct.unpack_from("<HH", b, 58)
    # (type, addr, offset, size, link) per section
    secs = [struct.unpack_from("<4xI8xQQQI", b, e_shoff + i * e_shentsize) for i in range(e_shnum)]
    syms = {}
    for s_type, _, s_off, s_size, s_link in secs:
        if s_type != 2:  # SHT_SYMTAB
            continue
        str_off = secs[s_link][2]
        for o in range(s_off, s_off + s_size, 24):
            st_name, st_info, _, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", b, o)
            if st_shndx == 0 or st_shndx >= e_shnum or (st_info & 15) not in (1, 2):
                continue  # only defined OBJECT / FUNC symbols
            end = b.index(b"\0", str_off + st_name)
            _, addr, off, _, _ = secs[st_shndx]
            start = off + st_value - (0 if e_type == 1 else addr)  # ET_REL: section-relative
            syms[b[str_off + st_name:end].decode()] = b[start:start + st_size]
    out = {}
    for name, kd in syms.items():
        if name.endswith(".kd") and len(kd) == 64 and name[:-3] in syms:
            out[name[:-3]] = (syms[name[:-3]], kd)
    return out


def demangle(names: list) -> list:
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:
        return names
    r = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True,
                       check=True)
    return r.stdout.splitlines()


def fingerprint_object(path: str) -> dict:
    """{demangled kernel name: {"code": sha256, "kd": sha256, "bytes": code size}}."""
    k = elf_kernels(path)
    names = sorted(k)
    out = {}
    for name, pretty in zip(names, demangle(names)):
        code, kd = k[name]
        kd = bytearray(kd)
        kd[KD_ENTRY_OFFSET] = bytes(8)
        out[pretty] = {"code": hashlib.sha256(code).hexdigest(),
                       "kd": hashlib.sha256(bytes(kd)).hexdigest(), "bytes": len(code)}
    return out


def device_flags(arch: str = "gfx950") -> list:
    """csrc/build.py's compile flags (kept in step with its build())."""
    return [f"--offload-arch={arch}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
            "-fno-fast-math", "-Wall", "-Wno-unused-result"]


def compile_device(hipcc: str, flags: list, src: str, obj: str) -> str:
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c",
                                          src, "-o", obj], capture_output=True, text=True)
    if r.returncode:  # warnings are the build's business; only a failure is shown
        raise RuntimeError(f"{src}: hipcc failed\n{r.stderr}")
    return obj


def fingerprint_tree(tree: str, only=()) -> dict:
    """{source file: fingerprint_object(...)} for every source of ``tree``'s build.py (or
    those named in ``only``)."""
    spec = importlib.util.spec_from_file_location(
        "_fp_build", os.path.join(tree, "rl4co_slap_amd", "csrc", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    flags = device_flags(bld.ARCH) + ["-I", os.path.join(tree, "include")]
    sources = [s for s in bld.SOURCES if not only or s in only]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=8) as ex:
        objs = list(ex.map(lambda s: compile_device(
            bld.hipcc(), flags, os.path.join(bld.HERE, s), os.path.join(tmp, s + ".o")),
            sources))
        return {s: fingerprint_object(o) for s, o in zip(sources, objs)}


def diff(old: dict, new: dict, renames: list) -> int:
    def flat(tree, subs=()):
        out = {}
        for src, kernels in tree.items():
            for name, fp in kernels.items():
                for pat, rep in subs:
                    name = re.sub(pat, rep, name)
                out[f"{src}: {name}"] = (fp["code"], fp["kd"])
        return out

    o, n = flat(old, [r.split("=>", 1) for r in renames]), flat(new)
    groups = [("only in OLD", sorted(set(o) - set(n))), ("only in NEW", sorted(set(n) - set(o))),
              ("changed", sorted(k for k in set(o) & set(n) if o[k] != n[k]))]
    print(f"kernels: OLD {len(o)}, NEW {len(n)}, identical {len(set(o) & set(n)) - len(groups[2][1])}")
    for title, names in groups:
        print(f"{title}: {len(names)}")
        for k in names:
            what = ""
            if title == "changed":
                what = "  [" + ", ".join(w for w, i in (("code", 0), ("kd", 1))
                                         if o[k][i] != n[k][i]) + "]"
            print(f"  {k}{what}")
    return 1 if any(names for _, names in groups) else 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT, help="repository tree to fingerprint")
    ap.add_argument("--source", action="append", default=[], metavar="FILE.hip",
                    help="fingerprint only this source (repeatable; default: all)")
    ap.add_argument("-o", "--out", help="write the JSON here instead of standard output")
    ap.add_argument("--diff", nargs=2, metavar=("OLD.json", "NEW.json"))
    ap.add_argument("--rename", action="append", default=[], metavar="'OLD=>NEW'",
                    help="regular-expression substitution on OLD's kernel names (with --diff)")
    a = ap.parse_args()
    if a.diff:
        with open(a.diff[0]) as f, open(a.diff[1]) as g:
            return diff(json.load(f), json.load(g), a.rename)
    text = json.dumps(fingerprint_tree(os.path.abspath(a.tree), a.source), indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
