"""Register spills of the library's kernels, from the code objects in libneo_hip.so (no GPU, no
compile): the .hip_fatbin section's offload bundles -> the gfx950 ELF of every translation unit ->
its AMDGPU metadata note (llvm-readelf --notes): per kernel .vgpr_count, .sgpr_count,
.vgpr_spill_count, .sgpr_spill_count, .private_segment_fixed_size, .group_segment_fixed_size.
Prints JSON; tests/test_abi.py asserts that the hot kernels spill nothing (a second inlined copy of
the slice roles once spilled 104 VGPRs in k_lvl_slices and cost the c5full step 12 %).

--diff OTHER.so: the kernel symbols whose machine-code bytes (size, SHA-256) or metadata differ
between this library and another build of it; exit status 1 if any does. The gate of a host-only
change: 0 differing. Bytes only, no instruction is decoded."""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(so_path):
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fatbin.bin")
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", so_path,
                        os.path.join(d, "x.so")], check=True, capture_output=True)
        blob = open(fb, "rb").read()
    out = []
    pos = blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + 24)[0]
        p = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + 1)
    return out


def metadata(co):
    """One code object's kernels: name -> the counts of its metadata note."""
    with tempfile.NamedTemporaryFile(suffix=".o") as f:
        f.write(co)
        f.flush()
        txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True,
                             text=True).stdout
    res = {}
    for block in txt.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        get = lambda k: int(re.search(rf"{k}:\s+(\d+)", block).group(1)) if re.search(rf"{k}:\s+(\d+)", block) else None
        res[name.group(1)] = {"vgpr": get(r"\.vgpr_count"), "sgpr": get(r"\.sgpr_count"),
                              "vgpr_spill": get(r"\.vgpr_spill_count"), "sgpr_spill": get(r"\.sgpr_spill_count"),
                              "scratch": get(r"\.private_segment_fixed_size"), "lds": get(r"\.group_segment_fixed_size")}
    return res


def kernels(so_path):
    res = {}
    for co in code_objects(so_path):
        res.update(metadata(co))
    return res


def symbol_bytes(co):
    """One code object's defined functions and objects (a kernel's code is the function NAME, its
    descriptor the object NAME.kd): symbol -> size and SHA-256 of its bytes. ELF64, little endian."""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    res = {}
    for _, kind, _, _, offset, size, link, _, _, _ in secs:
        if kind != 2:  # SHT_SYMTAB
            continue
        names = secs[link][4]
        for at in range(offset, offset + size, 24):
            name, info, _, shndx, value, nbytes = struct.unpack_from("<IBBHQQ", co, at)
            if info & 15 not in (1, 2) or not nbytes or not 0 < shndx < shnum or secs[shndx][1] == 8:  # SHT_NOBITS
                continue
            start = secs[shndx][4] + value - secs[shndx][3]
            sym = co[names + name:co.index(b"\0", names + name)].decode()
            res[sym] = {"size": nbytes, "sha256": hashlib.sha256(co[start:start + nbytes]).hexdigest()}
    return res


def diff(so_a, so_b):
    a, b = code_objects(so_a), code_objects(so_b)
    out = {"code_objects": [len(a), len(b)], "symbols": 0, "kernels": 0, "differing": []}
    for n, (x, y) in enumerate(zip(a, b)):
        for what, fx, fy in (("bytes", symbol_bytes(x), symbol_bytes(y)), ("metadata", metadata(x), metadata(y))):
            out["symbols" if what == "bytes" else "kernels"] += len(set(fx) | set(fy))
            out["differing"] += [{"code_object": n, "symbol": k, what: [fx.get(k), fy.get(k)]}
                                 for k in sorted(set(fx) | set(fy)) if fx.get(k) != fy.get(k)]
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    other = None
    if "--diff" in args:
        at = args.index("--diff")
        other = args[at + 1]
        del args[at:at + 2]
    so = args[0] if args else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                          "neo-dsp_amd", "lib", "libneo_hip.so")
    if other:
        d = diff(so, other)
        print(json.dumps(d, indent=1))
        sys.exit(1 if d["differing"] or d["code_objects"][0] != d["code_objects"][1] else 0)
    print(json.dumps(kernels(so), indent=1))
