"""Instructions in one trip of the hot loop of k_pbkdf2_sha512 (csrc/kdf.hpp), counted from the ISA listing of the built
library (no GPU needed).  Usage: python tools/kdf_loop_count.py [lib.so]
The hot loop is the kernel's longest backward branch: its body is one fully unrolled compression of a digest block.  Prints,
per instantiation, the loop's instructions by unit (VALU v_*, SALU s_*, other), its code bytes, and the VALU issue bound of
tools/bench_kdf.py: lanes x clock / (VALU per trip x trips per seed x cycles per wave64 VALU instruction / 64)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
CUS, SIMDS_PER_CU, SIMD_LANES, CLOCK_HZ = 256, 4, 32, 2.4e9       # the constants table of the MI355X microarchitecture guide
BIP39_TRIPS = 2 * (2048 - 1)                                       # compressions of the hot loop per seed


def listing(lib):
    with tempfile.TemporaryDirectory() as td:
        copy = os.path.join(td, "lib.so")
        shutil.copy(lib, copy)
        subprocess.check_output([f"{LLVM}/llvm-objdump", "--offloading", copy], cwd=td, text=True, stderr=subprocess.STDOUT)
        out = ""
        for f in os.listdir(td):
            if "gfx950" in f:
                out += subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--symbolize-operands", os.path.join(td, f)], text=True)
        return out


def hot_loops(text):
    """{kernel: (valu, salu, other, code bytes)} of the longest backward branch in every k_pbkdf2_sha512 instantiation"""
    found = {}
    for m in re.finditer(r"^[0-9a-f]+ <(_ZN3p2e15k_pbkdf2_sha512\w+)>:\n(.*?)(?=^[0-9a-f]+ <_Z|\Z)", text, flags=re.M | re.S):
        lines = [l for l in m.group(2).splitlines() if l.strip()]
        label_at, best = {}, None
        for k, l in enumerate(lines):
            lab = re.match(r"[0-9a-f]+ <(L\d+)>:", l.strip())
            if lab:
                label_at[lab.group(1)] = k
                continue
            br = re.match(r"\s*s_cbranch_\w+\s+(L\d+)", l)
            if br and br.group(1) in label_at and (best is None or k - label_at[br.group(1)] > best[1] - best[0]):
                best = (label_at[br.group(1)], k)
        body = [l.strip() for l in lines[best[0]:best[1] + 1] if not re.match(r"[0-9a-f]+ <", l.strip())]
        valu = sum(l.startswith("v_") for l in body)
        salu = sum(l.startswith("s_") for l in body)
        addr = lambda l: int(re.search(r"//\s*([0-9A-Fa-f]+):", l).group(1), 16)
        found[m.group(1)] = (valu, salu, len(body) - valu - salu, addr(body[-1]) + 4 - addr(body[0]))
    return found


def issue_bound(valu_per_trip, trips=BIP39_TRIPS):
    """seeds per second if every SIMD issued one wave64 VALU instruction every 2 cycles and nothing else cost anything"""
    lanes = CUS * SIMDS_PER_CU * SIMD_LANES
    return lanes * CLOCK_HZ / (valu_per_trip * trips)


if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "plonky2-ecdsa_amd", "libp2e_hip.so")
    for name, (valu, salu, other, size) in sorted(hot_loops(listing(lib)).items()):
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
        print(f"{dem}: hot loop {valu} VALU + {salu} SALU + {other} other instructions, {size} bytes of code; "
              f"VALU issue bound {issue_bound(valu) / 1e6:.2f} M seeds/s at 2048 iterations")
