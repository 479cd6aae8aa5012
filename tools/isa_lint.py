#!/usr/bin/env python3
"""ISA lint of the built library: no kernel may contain a packed-fp32 VALU instruction whose op_sel takes the HIGH half
of src1 for the low result lane (v_pk_mul_f32 / v_pk_add_f32 ... op_sel:[x,1], v_pk_fma_f32 ... op_sel:[x,1,x]).

On gfx950 that form reads the swizzled operand as zero while another wave of the same SIMD executes
v_mfma_f32_16x16x32_f16 (tools/probes/pk_opsel_mfma.hip) -- and the f16x2 field kernels without a time
encoding run that MFMA.  hipcc's SLP vectoriser is what emits the form, hence -fno-slp-vectorize in ced_nerf_amd/_lib.py;
this lint is the check that an edit or a flag change has not brought it back.  Second check: a K-doubled fp16 MFMA
(16x16x32 / 32x32x16) appears only in kernels that pass the residency gate of ced_nerf_amd/_k32_gate.py (their waves
hold all registers of their SIMDs, so no foreign wave can run beside them).
Usage: tools/isa_lint.py [library.so]   (exit status 1 and a list of kernels when either check fails)
"""
import os
import re
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
FORBIDDEN = re.compile(r"\b(v_pk_(?:mul|add|fma|min|max)_f32)\b[^\n]*?\bop_sel:\[[01],1"
                       # second rule (round 4): a multiply / fma folded into the fp32 -> fp16 conversion rounds ONCE to fp16;
                       # the CPU oracle (and the C standard) round to fp32 first.  field_half_device.hpp::to_half8 pins
                       # its inputs so that hipcc cannot form it; this keeps an edit from bringing it back.
                       # The ONE allowed use is the operand split's remainder, fp16(hi * m1 + x) with hi an fp16 source, m1 = -1.0
                       # in a scalar register and x an fp32 register (the fused result is the exact difference rounded once:
                       # tools/probes/split_mix_exhaustive.hip); a multiply folded by the compiler has fp32 sources.
                       r"|\bv_(?:fma|mad)_mix(?:lo|hi)_f16\b(?!\s+v\d+,\s*v\d+,\s*s\d+,\s*v\d+\s+(?:op_sel:\[1,0,0\]\s+)?op_sel_hi:\[1,0,0\])")


def code_objects(path):
    """the AMDGPU ELF images inside a HIP fat binary (.so)"""
    blob = open(path, "rb").read()
    starts = [m.start() for m in re.finditer(b"\x7fELF\x02\x01\x01\x40", blob)]
    for k, i in enumerate(starts):
        yield blob[i:starts[k + 1] if k + 1 < len(starts) else len(blob)]


def scan(path):
    """-> (number of kernels scanned, {kernel: [offending instruction lines]})"""
    bad, n_kernels = {}, 0
    for image in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(image)
            f.flush()
            text = subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True, check=True).stdout
        kernel = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                kernel = m.group(1)
                n_kernels += 1
                continue
            if FORBIDDEN.search(line):
                bad.setdefault(kernel, []).append(line.split("//")[0].strip())
    return n_kernels, bad


def k32_scan(path):
    """-> ({kernel: K-doubled fp16 MFMAs}, {kernel: why it fails the residency gate})"""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if here not in sys.path:
        sys.path.insert(0, here)
    from ced_nerf_amd import _k32_gate
    return _k32_gate.check(path)


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "ced_nerf_amd", "libcednerf_hip.so")
    n, bad = scan(path)
    print(f"{path}: {n} kernels scanned, {len(bad)} with a src1-high op_sel packed-fp32 instruction or a fused fp16-result fma")
    for k, lines in bad.items():
        print(f"  {k}: {len(lines)}   e.g. {lines[0]}")
    k32, ungated = k32_scan(path)
    print(f"{len(k32)} kernels with v_mfma_f32_16x16x32_f16 / 32x32x16_f16, {len(ungated)} of them without exclusive residency")
    for k, n_k32 in sorted(k32.items()):
        print(f"  {k}: {n_k32}" + (f"   FAILS: {ungated[k]}" if k in ungated else ""))
    return 1 if bad or ungated else 0


if __name__ == "__main__":
    sys.exit(main())
