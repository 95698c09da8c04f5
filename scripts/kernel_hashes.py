"""One line per gfx950 kernel of a built library: python scripts/kernel_hashes.py librtow_mi355x.so
(demangled name, code size in bytes, sha256 prefix of the kernel's bytes in .text; sorted by name, so two libraries diff line by line).
The code object comes out of the library's .hip_fatbin section; kernels are the FUNC symbols that have a `.kd` descriptor."""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def run(tool, *args):
    exe = shutil.which(tool) or os.path.join(LLVM, tool)
    return subprocess.run([exe, *args], check=True, capture_output=True, text=True).stdout


with tempfile.TemporaryDirectory() as tmp:
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, sys.argv[1], os.path.join(tmp, "rest.so"))
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co)
    # [Nr] Name Type Address Off Size ...: where .text lies in the file
    text = next(l.replace("[", " ").replace("]", " ").split() for l in run("llvm-readelf", "-SW", co).splitlines() if " .text " in l)
    text_nr, text_addr, text_off = text[0], int(text[3], 16), int(text[4], 16)
    syms = [l.split() for l in run("llvm-readelf", "-sW", co).splitlines()]
    syms = [f for f in syms if len(f) == 8 and f[0].endswith(":")]  # Num: Value Size Type Bind Vis Ndx Name
    kernels = {f[7][:-3] for f in syms if f[3] == "OBJECT" and f[7].endswith(".kd")}
    blob = open(co, "rb").read()
    rows = {}  # (.dynsym and .symtab both list a kernel)
    for f in syms:
        if f[3] == "FUNC" and f[6] == text_nr and f[7] in kernels:
            start, size = int(f[1], 16) - text_addr + text_off, int(f[2])
            rows[f[7]] = (size, hashlib.sha256(blob[start:start + size]).hexdigest()[:16])
names = run("c++filt", "-p", *rows).splitlines()
for name, (size, digest) in sorted(zip(names, rows.values())):
    print("%s  %d  %s" % (name, size, digest))
