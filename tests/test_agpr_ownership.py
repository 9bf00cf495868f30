"""CPU (hipcc cross-compiles): the kernels that name their AccVGPRs in the instruction strings own the whole AccVGPR file.

`dec_t2i_w1_kernel` keeps its 64 x 256 partial sums in a[0..255], `dec_i2t_w1_kernel` the prompt's folded K / V operands; the compiler is
told with a clobber list, but that is a statement about ONE point of the program: nothing stops the register allocator from parking a
VGPR it has no room for in a "free" AccVGPR (it prefers that to scratch), or from placing the result of an MFMA of its own there - both
were seen while these kernels were written (wrong results, no diagnostics).  So: compile the translation unit to assembly and require that
every AccVGPR reference of these kernels sits inside an inline-asm block (;;#ASMSTART .. ;;#ASMEND), that they use no scratch at all
(private segment 0, no scratch_ instruction), in BOTH operand-type builds (csrc/Makefile: op_bf16 and op_f16 are separate register
allocations of the same source), and that the two builds order their LDS-DMA traffic with the same counted waits (the same set of
s_waitcnt vmcnt immediates per kernel)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "saber_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BUILDS = {"op_bf16": ("_ZN7op_bf16", []), "op_f16": ("_ZN6op_f16", ["-DSABER_OP_F16=1"])}
_ASM = {}


def _asm(ns, tmp_path_factory):
    """decoder_fused.hip compiled to gfx950 assembly in the operand-type build `ns` (once per session)"""
    if ns not in _ASM:
        out = tmp_path_factory.mktemp(ns) / "decoder_fused.s"
        cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-result", "-Wno-unused-value", f"-DSABER_OP_NS={ns}",
               *BUILDS[ns][1], "-DSABER_OP_SRC=\"decoder_fused.hip\"", "-S", "--cuda-device-only", "op_wrap.hip", "-o", str(out)]
        r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        _ASM[ns] = out.read_text()
    return _ASM[ns]


def _w1_kernels(ns, text):
    """{mangled name without the namespace prefix: (function body, kernel descriptor)} of the six one-wave-per-SIMD instantiations"""
    prefix = BUILDS[ns][0]
    found = {}
    for m in re.finditer(r"^(" + prefix + r"(\d+(dec_t2i_w1_kernel|dec_i2t_w1_kernel)\w*)):", text, re.M):
        body = text[m.start():text.index(".Lfunc_end", m.start())]
        d0 = text.index(".amdhsa_kernel " + m.group(1) + "\n")
        desc = text[d0:text.index(".end_amdhsa_kernel", d0)]
        found[m.group(2)] = (body, desc)
    return found


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("ns", list(BUILDS))
def test_compiler_stays_out_of_the_accvgprs(tmp_path_factory, ns):
    kernels = _w1_kernels(ns, _asm(ns, tmp_path_factory))
    assert len(kernels) == 6, sorted(kernels)            # t2i_w1 <STAMPS, SHARED> x 4, i2t_w1 <SHARED> x 2
    for name, (body, desc) in kernels.items():
        inside, stray = False, []
        for line in body.split("\n"):
            if ";;#ASMSTART" in line:
                inside = True
            elif ";;#ASMEND" in line:
                inside = False
            elif not inside:
                code = line.split(";")[0]
                if "v_accvgpr" in code or re.search(r"\ba\[?\d", code):
                    stray.append(line.strip())
        assert not stray, (ns, name, stray[:5])
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", desc)
        assert seg and int(seg.group(1)) == 0, (ns, name, "private segment", seg and seg.group(1))
        assert "scratch_" not in body, (ns, name, "spills inside a one-wave-per-SIMD kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_both_builds_carry_the_same_counted_waits(tmp_path_factory):
    """the LDS-DMA ring of these kernels is ordered by counted vmcnt waits alone: a build whose compiler re-ordered, merged or dropped one
    would show a different set of immediates"""
    sets = {}
    for ns in BUILDS:
        sets[ns] = {name: sorted({int(v) for v in re.findall(r"s_waitcnt\s[^\n;]*vmcnt\((\d+)\)", body)})
                    for name, (body, desc) in _w1_kernels(ns, _asm(ns, tmp_path_factory)).items()}
    for name in sorted(sets["op_bf16"]):
        print(name[:60], sets["op_bf16"][name])
    assert sets["op_bf16"] == sets["op_f16"]
    assert all(len(v) > 1 for v in sets["op_bf16"].values())
