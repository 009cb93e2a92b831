#!/usr/bin/env python3
"""One line per gfx950 kernel of a built library or kernel pack: registers, spills, LDS, scratch, instruction count and a hash of
its disassembly -- sorted by name, so that `diff` of two digests says whether two builds hold the same device code whatever the
order their kernels were emitted in.

    python tools/codeobj_digest.py libdwbc_amd/libdwbc_hip.so > a.txt     (needs no GPU; uses the LLVM tools of ROCm)
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "copy")])
    data = open(fat, "rb").read()
    starts = sorted(m.start() for magic in MAGICS for m in re.finditer(re.escape(magic), data))
    # a compressed bundle holds no plain magic inside; a plain one is never nested: every hit starts one translation unit's bundle
    for i, a in enumerate(starts):
        part = os.path.join(tmp, f"bundle{i}")
        open(part, "wb").write(data[a:starts[i + 1] if i + 1 < len(starts) else len(data)])
        out = os.path.join(tmp, f"tu{i}.co")
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part, "--targets=" + TARGET, "--output=" + out])
        if os.path.getsize(out):
            yield out


def kernels(co):
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    meta = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        get = lambda key: re.search(r"\.%s:\s+(\S+)" % key, block).group(1)
        meta[get("name")] = " ".join(f"{k}={get(v)}" for k, v in (("vgpr", "vgpr_count"), ("vgpr_spill", "vgpr_spill_count"), ("sgpr", "sgpr_count"), ("sgpr_spill", "sgpr_spill_count"),
                                                                 ("lds", "group_segment_fixed_size"), ("scratch", "private_segment_fixed_size")))
        meta[get("name")] = "agpr=" + block.split()[0] + " " + meta[get("name")]
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    body = {}
    name = None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            name = m.group(1)
            body[name] = []
        elif name and line.strip() and line.strip() != "...":  # ("...": zero padding behind whichever kernel comes last in the section)
            body[name].append(line.split("//")[0].strip())
    for k, v in meta.items():
        text = body.get(k, [])
        yield k, f"{v} insns={len(text)} sha1={hashlib.sha1(chr(10).join(text).encode()).hexdigest()[:16]}"


def main():
    with tempfile.TemporaryDirectory() as tmp:
        rows = sorted(r for co in code_objects(sys.argv[1], tmp) for r in kernels(co))
    filt = shutil.which("c++filt")  # readable names where binutils is installed
    names = subprocess.check_output([filt], input="\n".join(r[0] for r in rows), text=True).splitlines() if filt and rows else [r[0] for r in rows]
    for name, (_, info) in zip(names, rows):
        print(name, info)
    print(f"# {len(rows)} kernels")


if __name__ == "__main__":
    main()
