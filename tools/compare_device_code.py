"""Compare the gfx950 device code of two object directories, unit by unit.

    python tools/compare_device_code.py PARENT/zigma_amd/build HEAD/zigma_amd/build

For each *.o: the .hip_fatbin section is unbundled for gfx950, disassembled with llvm-objdump -d, and the two texts
are compared line by line.  One `name identical|DIFFERS (N lines)` line per unit; the exit status is 1 on any
difference.  Objects without device code (api.o) are skipped."""
import glob
import os
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def disassembly(obj, tmp):
    """lines of `llvm-objdump -d` of obj's gfx950 code object (without the header line that names the file), or None when it has none"""
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fatbin], check=True)
    if not os.path.exists(fatbin) or os.path.getsize(fatbin) == 0:
        return None
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET,
                    "--input=" + fatbin, "--output=" + co], check=True)
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout
    os.remove(fatbin)
    return [ln for ln in out.splitlines() if "file format" not in ln]


def main(dir_a, dir_b):
    names = sorted({os.path.basename(p)[:-2] for d in (dir_a, dir_b) for p in glob.glob(os.path.join(d, "*.o"))})
    differs = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in names:
            paths = [os.path.join(d, name + ".o") for d in (dir_a, dir_b)]
            if not all(map(os.path.exists, paths)):
                print(f"{name} DIFFERS (missing on one side)")
                differs += 1
                continue
            a, b = (disassembly(p, tmp) for p in paths)
            if a is None and b is None:
                continue
            a, b = a or [], b or []
            n = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
            differs += n != 0
            print(f"{name} DIFFERS ({n} lines)" if n else f"{name} identical ({len(a)} lines of disassembly)")
    return 1 if differs else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
