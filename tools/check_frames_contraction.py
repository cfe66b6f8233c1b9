#!/usr/bin/env python3
"""Do the frame-writing flow kernels round like their mode-0 twins?  (csrc/ff_dp5.h, PIN_B)

CNF.generate(z, nframes = 2) promises the bits of CNF.generate(z): ff_ode_fwd_kernel<N, D, FF_MODE_FRAMES, TAB> and
ff_wide_flow_kernel<D, FF_MODE_FRAMES, TAB> are the mode-0 kernels with another stepper.  The Dormand-Prince sums
(A40 k0 + A41 k1 + ..., B0 k0 + B2 k2 + B3 k3, E0 k0 + ...) are written as plain sums and contracted by the compiler
(-ffp-contract=fast) into one multiplication and a chain of fused multiply-adds; WHICH product stays the multiplication is
the compiler's choice per instantiation, and it is one rounding of the result.  hipcc 7.2 chooses alike for every narrow
pair and differently for the wide pairs, which is why ff_wide.hip pins the choice of its frame-writing kernels (PIN_B).

This tool reads the choice off the built library: for every kernel of the two families the Dormand-Prince coefficient that
each v_mul_f64 / v_fma_f64 / v_fmac_f64 carries as a literal, as a multiset, and compares each frame-writing kernel with its twin.
After a toolchain update that breaks tests/test_gpu_frames.py::test_frame_zero_and_two_frames, run it: the report names the
kernels and the coefficient whose product is the multiplication in the twin -- B2: PIN_B = 1, B0: PIN_B = 2 in ff_wide.hip;
another sum, or a narrow kernel, needs the same treatment in the source it names.

usage: check_frames_contraction.py fermiflow_amd/libfermiflow_hip.so       (exit status 1 on a mismatch; seconds)
       tests/test_frames_host.py runs exactly that on the built library."""
import collections
import os
import re
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_agpr_spills import parse_library      # noqa: E402

COEFF = {"A10": 1 / 5, "A20": 3 / 40, "A21": 9 / 40, "A30": 44 / 45, "A31": -56 / 15, "A32": 32 / 9, "A40": 19372 / 6561, "A41": -25360 / 2187,
         "A42": 64448 / 6561, "A43": -212 / 729, "A50": 9017 / 3168, "A51": -355 / 33, "A52": 46732 / 5247, "A53": 49 / 176, "A54": -5103 / 18656,
         "B0": 35 / 384, "B2": 500 / 1113, "B3": 125 / 192, "B4": -2187 / 6784, "B5": 11 / 84, "E0": -71 / 57600, "E2": 71 / 16695,
         "E3": -71 / 1920, "E4": 17253 / 339200, "E5": -22 / 525, "E6": 1 / 40}
BY_BITS = {}
for _k, _v in COEFF.items():
    for _sign, _val in (("", _v), ("-", -_v)):
        BY_BITS[struct.unpack("<Q", struct.pack("<d", _val))[0]] = _sign + _k
FRAMES = 3      # FF_MODE_FRAMES (csrc/ff_fwd_args.h)
TWIN = re.compile(r"^(_Z17ff_ode_fwd_kernelILi\d+ELi\dE|_Z19ff_wide_flow_kernelILi\dE)Li(\d)E(Lb[01]E.*)$")


def signature(items):
    """multiset of (opcode, coefficient) over the fp64 multiplications and fused multiply-adds that carry a coefficient literal"""
    sreg, sig = {}, collections.Counter()
    for kind, s in items:
        if kind != "ins":
            continue
        s = s.replace("vcc_lo", "s106").replace("vcc_hi", "s107")
        s = re.sub(r"\bvcc\b", "s[106:107]", s)
        m = re.match(r"s_mov_b32 s(\d+), (0x[0-9a-fA-F]+|-?\d+)$", s)
        if m:
            sreg[int(m.group(1))] = int(m.group(2), 0) & 0xffffffff
            continue
        m = re.match(r"s_mov_b64 s\[(\d+):(\d+)\], (0x[0-9a-fA-F]+|-?\d+)$", s)
        if m:
            v = int(m.group(3), 0) & 0xffffffffffffffff
            sreg[int(m.group(1))], sreg[int(m.group(2))] = v & 0xffffffff, v >> 32
            continue
        m = re.match(r"s_\w+ s(\d+),", s)
        if m:
            sreg.pop(int(m.group(1)), None)
        m = re.match(r"s_\w+ s\[(\d+):(\d+)\],", s)
        if m:
            for k in range(int(m.group(1)), int(m.group(2)) + 1):
                sreg.pop(k, None)
        op = s.split()[0]
        if not re.match(r"v_(mul|fma|fmac)_f64", op):
            continue
        for lo, hi in re.findall(r"s\[(\d+):(\d+)\]", s):
            lo, hi = int(lo), int(hi)
            if lo in sreg and hi in sreg and ((sreg[hi] << 32) | sreg[lo]) in BY_BITS:
                sig[(re.sub(r"_e(32|64)$", "", op), BY_BITS[(sreg[hi] << 32) | sreg[lo]])] += 1
    return sig


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    funcs = parse_library(sys.argv[1])
    pairs, bad = 0, 0
    for name, items in sorted(funcs.items()):
        m = TWIN.match(name)
        if not m or int(m.group(2)) != FRAMES:
            continue
        twin = m.group(1) + "Li0E" + m.group(3)
        if twin not in funcs:
            print("%s: no mode-0 twin in the library" % name)
            bad += 1
            continue
        pairs += 1
        a, b = signature(funcs[twin]), signature(items)
        if not a:
            print("%s: no coefficient literal found -- the disassembly is not what this tool reads" % twin)
            bad += 1
        elif a != b:
            bad += 1
            print("%s rounds unlike %s:" % (name, twin))
            for key in sorted(set(a) | set(b)):
                if a[key] != b[key]:
                    print("    %-12s %-4s  twin %d  frames %d" % (key[0], key[1], a[key], b[key]))
    print("%d pair(s) of kernels compared, %d differ" % (pairs, bad))
    return 1 if bad or not pairs else 0


if __name__ == "__main__":
    sys.exit(main())
