"""The tabulated flow kernels keep the register budget of four waves per SIMD (csrc/ff_cnf_fwd.hip FF_FLOW_WAVES): from the
code-object metadata of the BUILT libfermiflow_hip.so (no GPU, nothing compiled here), every ff_ode_fwd_kernel<N, D, 0 | FRAMES, true>
the launch bound names -- N * D <= 12 -- has vgpr_count + agpr_count <= 128 and no scratch.  A launch bound alone does not give that:
the allocator meets it by spilling (the kernel was 128 registers + 44 B of scratch per lane before its diet), and an unrelated change
once moved the three-wave kernel from 159 to 169 registers unnoticed (two waves, 112 -> 143 us).  Skips if the library was not built
for gfx950 or the LLVM tools are not there."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fermiflow_amd", "libfermiflow_hip.so")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
FF_MODE_FRAMES = 3                      # csrc/ff_fwd_args.h
FOUR_WAVE_BUDGET = 128                  # 512 registers per SIMD lane, four waves
# the shapes the dispatch instantiates under the bound (csrc/ff_cnf_fwd.hip: N * D <= 12)
SHAPES = [(n, 2) for n in range(1, 7)] + [(2, 3), (3, 3), (4, 3)]
ENTRY = re.compile(r"- \.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?"
                   r"\.vgpr_spill_count:\s+(\d+)", re.S)


def kernel_metadata(lib):
    """{mangled kernel name: (vgprs, agprs, scratch bytes, spilled vgprs)} of the gfx950 code objects embedded in the library"""
    data = open(lib, "rb").read()
    starts = [m.start() for m in re.finditer(b"\x7fELF", data)][1:]          # [0] is the host ELF itself
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, st in enumerate(starts):
            co = os.path.join(tmp, "co%d.elf" % k)
            with open(co, "wb") as f:
                f.write(data[st:starts[k + 1] if k + 1 < len(starts) else len(data)])
            r = subprocess.run([READELF, "--notes", co], capture_output=True, text=True)
            if r.returncode != 0 or "gfx950" not in r.stdout:
                continue
            for ag, name, scr, vg, sp in ENTRY.findall(r.stdout):
                out[name] = (int(vg), int(ag), int(scr), int(sp))
    return out


def test_tabulated_flow_kernels_fit_four_waves_without_scratch():
    if not os.path.exists(LIB) or not os.path.exists(READELF):
        pytest.skip("library or llvm-readelf not present")
    meta = kernel_metadata(LIB)
    if not meta:
        pytest.skip("no gfx950 code object in the library")
    seen, over = [], {}
    for n, d in SHAPES:
        for mode in (0, FF_MODE_FRAMES):
            name = f"_Z17ff_ode_fwd_kernelILi{n}ELi{d}ELi{mode}ELb1EEv11ff_fwd_args"
            assert name in meta, f"{name} is not in the library"
            vg, ag, scr, sp = meta[name]
            seen.append((n, d, mode, vg, ag, scr))
            if vg + ag > FOUR_WAVE_BUDGET or scr != 0 or sp != 0:
                over[n, d, mode] = (vg, ag, scr, sp)
    print("FLOWWAVES registers (n, d, mode, vgpr, agpr, scratch):", seen)
    assert not over, over
